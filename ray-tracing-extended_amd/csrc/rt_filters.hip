// rt_filters.hip — the image filters' one host path: rt_denoise, rt_temporal, rt_denoise_temporal, rt_denoise_variance, the
// reads of their planes, and the same calls for the rt_multi handle, whose two halves of the path are rt_multi.hip's.
#include <cmath>
#include <initializer_list>

#include "rt_ctx.hpp"
#include "rt_denoise.hpp"
#include "rt_temporal.hpp"
#include "rt_vdenoise.hpp"

namespace rth __attribute__((visibility("hidden"))) {       // (hidden here as in rt_ctx.hpp: the *_call<rt_ctx> instantiations are this block's)

// ---- the image filters' one host path -----------------------------------------------------------------------------------
// rt_denoise, rt_temporal, rt_denoise_temporal, rt_denoise_variance and their rt_multi_ forms are each: begin_filter, the filter's
// validator, filter_inputs, the filter's run_*.  A context and a handle differ in the two overloads of begin_filter and filter_inputs (and
// in the order of their checks); everything else below is written once.

// The temporal colour as a filter's source: T exists and has the image's size.  `temporal` is the call that makes T and `whose` the
// owner of the image in the messages ("context's" / "handle's")
int temporal_source(ErrOwner* o, const TemporalPlanes& T, int W, int H, const FilterCall& k, const char* temporal, const char* whose)
{
    if (!T.filled) return fail(o, -2, "%s: %s%s has not been called", k.what, k.lead, temporal);
    if (T.w != W || T.h != H) return fail(o, -2, "%s: the temporal image is %d x %d, the %s image %d x %d", k.what, T.w, T.h, whose, W, H);
    return 0;
}

namespace {

// A context may run the call: settled, with params ...
int begin_filter(rt_ctx* c, const char* what)
{
    RT_SETTLE(c);
    return c->have_params ? 0 : fail(c, -2, "%s: rt_set_params has not been called", what);
}
// ... and it holds the whole image and current feature planes with a frame in them (planes of another layout would be re-created,
// zeroed); then T, if that is the source (from_T) and not the image; then the inputs on its device (the image is a cleared one if it was
// never created at this size)
int filter_inputs(rt_ctx* c, const FilterCall& k, bool from_T, FilterInputs& I)
{
    StripLayout L;
    { int r = strip_layout(c, L); if (r) return r; }
    if (c->band_stride > 1 || L.row0 != 0 || L.rows != L.h)
        return fail(c, -2, "%s: the context holds rows of the image, not the whole image (%d of %d rows); use %s", k.what, L.rows, L.h, k.use_instead);
    if (!aov_current(c, L) || c->aov_info.framesAccumulated == 0) return fail(c, -2, "%s: no feature frame accumulated (call rt_render_aov first)", k.what);
    if (from_T) { int r = temporal_source(c, c->tp, L.w, L.h, k, "rt_temporal", "context's"); if (r) return r; }
    RT_HIP(c, hipSetDevice(c->device));
    if (!from_T) { int r = ensure_targets(c); if (r) return r; }
    I.C = from_T ? c->tp.t[c->tp.cur].p : c->d_accum.p; I.A = c->d_aov[RT_AOV_ALBEDO].p; I.G = c->d_aov[RT_AOV_NORMAL_DEPTH].p;
    I.W = L.w; I.H = L.h; I.cam = &c->params;
    I.stream = c->stream; I.ev0 = c->ev_dn0; I.ev1 = c->ev_dn1;
    return 0;
}
// (the handle's two: rt_multi.hip)

// `launches` on `stream` between ev0 and ev1, waited for -> their time
template <class Fn> hipError_t timed(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, float& ms, Fn launches)
{
    hipError_t e;
    if ((e = hipEventRecord(ev0, stream)) != hipSuccess) return e;
    launches();
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipEventRecord(ev1, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    return hipEventElapsedTime(&ms, ev0, ev1);
}

// The pieces the validators are made of.  A validator gives P the caller's parameters or the defaults, and returns nullptr, or why they
// are out of range
bool is_flag(int v) { return v == 0 || v == 1; }
bool finite_and_positive(std::initializer_list<float> values)
{
    for (float v : values) if (!std::isfinite(v) || !(v > 0.0f)) return false;
    return true;
}
const char* atrous_params(int iterations, int demodulate)           // what both A-trous filters take
{
    if (iterations < 1 || iterations > 6) return "iterations outside 1..6";
    return is_flag(demodulate) ? nullptr : "demodulate is neither 0 nor 1";
}

// The readers of a filter's plane S (`call`: the call that fills it), for the owner o whose plane it is, on the context `on` that holds
// it (copy_plane).  `per` floats per pixel: 4 or 1
int readable(ErrOwner* o, const FilterPlanes& S, const char* call, const void* dst)
{
    if (!S.filled) return fail(o, -2, "%s has not been called", call);
    return dst ? 0 : fail(o, -2, "null destination");
}

} // namespace

int read_filter_plane(ErrOwner* o, const rt_ctx* on, const FilterPlanes& S, const char* call, const void* src, int per, void* dst, size_t n_floats, bool to_device)
{
    { int r = readable(o, S, call, dst); if (r) return r; }
    return copy_plane(o, on, src, S.pixels() * per, per == 4 ? "height*width*4" : "height*width", dst, n_floats, to_device);
}
// ... as sRGB8, through the display step (read_srgb8, rt_api.hip)
int read_filter_display(ErrOwner* o, rt_ctx* on, const FilterPlanes& S, const char* call, const float4* plane, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels)
{
    { int r = readable(o, S, call, rgba8); if (r) return r; }
    return read_srgb8(o, on, plane, S.pixels(), display, rgba8, n_pixels);
}

namespace {

// a context's reads of its own filter planes (the queue settled first)
enum class OwnPlane { Denoised, Temporal, History, Variance };
int read_own(rt_ctx* c, OwnPlane which, void* dst, size_t n_floats, bool to_device)
{
    if (!c) return -1;
    RT_SETTLE(c);
    switch (which) {
    case OwnPlane::Denoised: return read_filter_plane(c, c, c->dn, "rt_denoise", c->dn.out.p, 4, dst, n_floats, to_device);
    case OwnPlane::Temporal: return read_filter_plane(c, c, c->tp, "rt_temporal", c->tp.t[c->tp.cur].p, 4, dst, n_floats, to_device);
    case OwnPlane::History:  return read_filter_plane(c, c, c->tp, "rt_temporal", c->tp.n[c->tp.cur].p, 1, dst, n_floats, to_device);
    default:                 return read_filter_plane(c, c, c->vd, "rt_denoise_variance", c->vd.var.p, 1, dst, n_floats, to_device);
    }
}

// ---- denoiser (rt_denoise, csrc/rt_denoise.hpp) -----------------------------------------------------------------------------------
static_assert(sizeof(rt_denoise_params) == 32 && sizeof(rt_denoise_info) == 32, "denoiser ABI");

const char* denoise_params(const rt_denoise_params* in, rt_denoise_params& P)
{
    P = rt_denoise_params{};
    P.iterations = RT_DENOISE_DEFAULT_ITERATIONS; P.demodulate = RT_DENOISE_DEFAULT_DEMODULATE;
    P.sigmaColour = RT_DENOISE_DEFAULT_SIGMA_COLOUR; P.sigmaNormal = RT_DENOISE_DEFAULT_SIGMA_NORMAL; P.sigmaDepth = RT_DENOISE_DEFAULT_SIGMA_DEPTH;
    if (in) P = *in;
    if (const char* why = atrous_params(P.iterations, P.demodulate)) return why;
    return finite_and_positive({ P.sigmaColour, P.sigmaNormal, P.sigmaDepth }) ? nullptr : "a sigma is not finite or not > 0";
}

// What both A-trous filters start with (inside their timed launches): e_0 and d from C and A, then the passes' tile grid and the
// guide weights' factors
struct AtrousStart { dim3 grid; float kn, kz; };
AtrousStart atrous_start(DenoisePlanes& D, const FilterInputs& I, int demodulate, float sigmaNormal, float sigmaDepth)
{
    const size_t px = I.pixels();
    hipLaunchKernelGGL(rtk::k_denoise_prep, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, I.stream, I.C, I.A, D.e[0].p, D.d.p, px, demodulate);
    return { dim3((I.W + rtk::kDenoiseTileW - 1) / rtk::kDenoiseTileW, (I.H + rtk::kDenoiseTileH - 1) / rtk::kDenoiseTileH),
             1.0f / (sigmaNormal * sigmaNormal), 1.0f / (sigmaDepth * sigmaDepth) };
}

// The filter: I -> D.out; P has passed denoise_params
hipError_t run_denoise(DenoisePlanes& D, const FilterInputs& I, const rt_denoise_params& P)
{
    hipError_t e = D.at(I.W, I.H);
    if (e != hipSuccess) return e;
    float ms = 0.f;
    if (I.pixels()) e = timed(I.stream, I.ev0, I.ev1, ms, [&] {
        const AtrousStart s = atrous_start(D, I, P.demodulate, P.sigmaNormal, P.sigmaDepth);
        const float kc0 = 1.0f / (P.sigmaColour * P.sigmaColour);
        for (int i = 0; i < P.iterations; ++i) {
            const bool last = i == P.iterations - 1;
            rtk::AtrousArgs a{};
            a.e_in = D.e[i & 1].p; a.guide = I.G; a.d = D.d.p; a.e_out = last ? D.out.p : D.e[(i + 1) & 1].p;
            a.W = I.W; a.H = I.H; a.step = 1 << i;
            a.kn = s.kn; a.kz = s.kz; a.kc = kc0 * (float)(1 << (2 * i));
            if (last) hipLaunchKernelGGL(rtk::k_atrous<true>, s.grid, dim3(256), 0, I.stream, a);
            else hipLaunchKernelGGL(rtk::k_atrous<false>, s.grid, dim3(256), 0, I.stream, a);
        }
    });
    if (e != hipSuccess) return e;
    D.filled = true;
    D.info.iterations = P.iterations; D.info.demodulate = P.demodulate; D.info.width = I.W; D.info.height = I.H;
    D.info.lastKernelMs = ms; D.info.totalKernelMs += ms;
    return hipSuccess;
}

} // namespace

// rt_denoise, rt_denoise_temporal (from_T) and their rt_multi_ forms
template <class Owner> int denoise_call(Owner* o, const FilterCall& k, bool from_T, const rt_denoise_params* in)
{
    if (!o) return -1;
    { int r = begin_filter(o, k.what); if (r) return r; }
    rt_denoise_params P;
    if (const char* why = denoise_params(in, P)) return fail(o, -2, "%s: %s", k.what, why);
    FilterInputs I;
    { int r = filter_inputs(o, k, from_T, I); if (r) return r; }
    RT_HIP(o, run_denoise(o->dn, I, P));
    return 0;
}
template int denoise_call(rt_multi*, const FilterCall&, bool, const rt_denoise_params*);

namespace {

// ---- temporal reprojection (rt_temporal, csrc/rt_temporal.hpp) --------------------------------------------------------------------
static_assert(sizeof(rt_temporal_params) == 32 && sizeof(rt_temporal_info) == 32, "temporal ABI");

const char* temporal_params(const rt_temporal_params* in, rt_temporal_params& P)
{
    P = rt_temporal_params{};
    P.maxHistory = RT_TEMPORAL_DEFAULT_MAX_HISTORY;
    P.depthTolerance = RT_TEMPORAL_DEFAULT_DEPTH_TOLERANCE; P.normalTolerance = RT_TEMPORAL_DEFAULT_NORMAL_TOLERANCE;
    if (in) P = *in;
    if (P.maxHistory < 1 || P.maxHistory > 4096) return "maxHistory outside 1..4096";
    return finite_and_positive({ P.depthTolerance, P.normalTolerance }) ? nullptr : "a tolerance is not finite or not > 0";
}

// The step: I (and its camera) -> the other pair of S's planes; P has passed temporal_params.  Without history (call 0) N' is zeroed, so
// no tap counts, and the previous camera is this call's.
hipError_t run_temporal(TemporalPlanes& S, const FilterInputs& I, const rt_temporal_params& P)
{
    const size_t px = I.pixels();
    const rt_params& cam = *I.cam;
    hipError_t e = S.at(I.W, I.H);
    if (e != hipSuccess) return e;
    const int prev = S.cur, next = S.cur ^ 1;
    float ms = 0.f;
    if (px) {
        if (!S.filled) {            // no history: T', N' and G' read as zero
            if ((e = hipMemsetAsync(S.t[prev].p, 0, px * sizeof(float4), I.stream)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(S.g[prev].p, 0, px * sizeof(float4), I.stream)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(S.n[prev].p, 0, px * sizeof(float), I.stream)) != hipSuccess) return e;
        }
        const rt_params& pc = S.filled ? S.cam : cam;
        rtk::TemporalArgs a{};
        a.C = I.C; a.A = I.A; a.G = I.G;
        a.Tp = S.t[prev].p; a.Np = S.n[prev].p; a.Gp = S.g[prev].p;
        a.T = S.t[next].p; a.N = S.n[next].p; a.Gn = S.g[next].p;
        a.W = I.W; a.H = I.H;
        for (int i = 0; i < 12; ++i) a.M[i] = cam.camLocalToWorld[i];
        const float* Mp = pc.camLocalToWorld;
        for (int i = 0; i < 3; ++i) {
            a.O[i] = cam.worldSpaceCameraPos[i]; a.V[i] = cam.viewParams[i];
            a.pO[i] = pc.worldSpaceCameraPos[i]; a.pV[i] = pc.viewParams[i];
            a.pt[i] = Mp[4 * i + 3];
            const float cx = Mp[i], cy = Mp[4 + i], cz = Mp[8 + i];
            a.pc[i][0] = cx; a.pc[i][1] = cy; a.pc[i][2] = cz;
            a.pcc[i] = (cx * cx + cy * cy) + cz * cz;
        }
        a.depthTol = P.depthTolerance; a.normalTol2 = P.normalTolerance * P.normalTolerance; a.maxHistory = (float)P.maxHistory;
        const dim3 grid((I.W + rtk::kTemporalTileW - 1) / rtk::kTemporalTileW, (I.H + rtk::kTemporalTileH - 1) / rtk::kTemporalTileH);
        if ((e = timed(I.stream, I.ev0, I.ev1, ms, [&] { hipLaunchKernelGGL(rtk::k_temporal, grid, dim3(256), 0, I.stream, a); })) != hipSuccess) return e;
    }
    S.cur = next; S.filled = true; S.cam = cam;
    S.info.calls += 1; S.info.width = I.W; S.info.height = I.H;
    S.info.lastKernelMs = ms; S.info.totalKernelMs += ms;
    return hipSuccess;
}

} // namespace

// rt_temporal and rt_multi_temporal
template <class Owner> int temporal_call(Owner* o, const FilterCall& k, const rt_temporal_params* in)
{
    if (!o) return -1;
    { int r = begin_filter(o, k.what); if (r) return r; }
    rt_temporal_params P;
    if (const char* why = temporal_params(in, P)) return fail(o, -2, "%s: %s", k.what, why);
    FilterInputs I;
    { int r = filter_inputs(o, k, false, I); if (r) return r; }
    RT_HIP(o, run_temporal(o->tp, I, P));
    return 0;
}
template int temporal_call(rt_multi*, const FilterCall&, const rt_temporal_params*);

namespace {

// ---- variance-guided denoiser (rt_denoise_variance, csrc/rt_vdenoise.hpp) -----------------------------------------------------------
static_assert(sizeof(rt_vdenoise_params) == 32 && sizeof(rt_vdenoise_info) == 32, "variance-guided denoiser ABI");

const char* vdenoise_params(const rt_vdenoise_params* in, rt_vdenoise_params& P)
{
    P = rt_vdenoise_params{};
    P.iterations = RT_VDENOISE_DEFAULT_ITERATIONS; P.demodulate = RT_VDENOISE_DEFAULT_DEMODULATE;
    P.sigmaLuminance = RT_VDENOISE_DEFAULT_SIGMA_LUMINANCE; P.sigmaNormal = RT_VDENOISE_DEFAULT_SIGMA_NORMAL; P.sigmaDepth = RT_VDENOISE_DEFAULT_SIGMA_DEPTH;
    if (in) P = *in;
    if (const char* why = atrous_params(P.iterations, P.demodulate)) return why;
    if (!is_flag(P.source)) return "source is neither 0 nor 1";
    if (!finite_and_positive({ P.sigmaLuminance, P.sigmaNormal, P.sigmaDepth })) return "a sigma is not finite or not > 0";
    return P._reserved[0] == 0 && P._reserved[1] == 0 ? nullptr : "a reserved word is not 0";
}

// The filter: I -> D.out and V.var, through D's work planes; P has passed vdenoise_params
hipError_t run_vdenoise(DenoisePlanes& D, VariancePlane& V, const FilterInputs& I, const rt_vdenoise_params& P)
{
    hipError_t e;
    if ((e = D.at(I.W, I.H)) != hipSuccess || (e = V.at(I.W, I.H)) != hipSuccess) return e;
    float ms = 0.f;
    if (I.pixels()) e = timed(I.stream, I.ev0, I.ev1, ms, [&] {
        const AtrousStart s = atrous_start(D, I, P.demodulate, P.sigmaNormal, P.sigmaDepth);
        rtk::VarEstimateArgs v{};
        v.e0 = D.e[0].p; v.guide = I.G; v.e_out = D.e[1].p; v.var = V.var.p; v.W = I.W; v.H = I.H; v.kn = s.kn; v.kz = s.kz;
        hipLaunchKernelGGL(rtk::k_variance_estimate, s.grid, dim3(256), 0, I.stream, v);
        for (int i = 0; i < P.iterations; ++i) {            // (e_0, var_0) is in e[1]: pass i reads e[(i + 1) & 1]
            const bool last = i == P.iterations - 1;
            rtk::VarAtrousArgs a{};
            a.e_in = D.e[(i + 1) & 1].p; a.guide = I.G; a.d = D.d.p; a.e_out = last ? D.out.p : D.e[i & 1].p;
            a.W = I.W; a.H = I.H; a.step = 1 << i;
            a.kn = s.kn; a.kz = s.kz; a.sl = P.sigmaLuminance;
            if (last) hipLaunchKernelGGL(rtk::k_var_atrous<true>, s.grid, dim3(256), 0, I.stream, a);
            else hipLaunchKernelGGL(rtk::k_var_atrous<false>, s.grid, dim3(256), 0, I.stream, a);
        }
    });
    if (e != hipSuccess) return e;
    D.filled = true; V.filled = true;
    V.info.iterations = P.iterations; V.info.source = P.source; V.info.width = I.W; V.info.height = I.H;
    V.info.lastKernelMs = ms; V.info.totalKernelMs += ms;
    return hipSuccess;
}

} // namespace

// rt_denoise_variance and rt_multi_denoise_variance (source 1: the temporal colour)
template <class Owner> int denoise_variance_call(Owner* o, const FilterCall& k, const rt_vdenoise_params* in)
{
    if (!o) return -1;
    { int r = begin_filter(o, k.what); if (r) return r; }
    rt_vdenoise_params P;
    if (const char* why = vdenoise_params(in, P)) return fail(o, -2, "%s: %s", k.what, why);
    FilterInputs I;
    { int r = filter_inputs(o, k, P.source == 1, I); if (r) return r; }
    RT_HIP(o, run_vdenoise(o->dn, o->vd, I, P));
    return 0;
}
template int denoise_variance_call(rt_multi*, const FilterCall&, const rt_vdenoise_params*);

} // namespace rth

using namespace rth;

extern "C" {

int rt_denoise(rt_ctx* c, const rt_denoise_params* params) { return denoise_call(c, { "rt_denoise", "rt_multi_denoise" }, false, params); }
int rt_read_denoised(rt_ctx* c, float* rgba, size_t n) { return read_own(c, OwnPlane::Denoised, rgba, n, false); }
int rt_copy_denoised_to_device(rt_ctx* c, void* dst, size_t n) { return read_own(c, OwnPlane::Denoised, dst, n, true); }
int rt_read_denoised_display(rt_ctx* c, uint32_t* rgba8, size_t n_pixels)
{
    if (!c) return -1;
    RT_SETTLE(c);
    return read_filter_display(c, c, c->dn, "rt_denoise", c->dn.out.p, c->d_display, rgba8, n_pixels);
}
int rt_get_denoise_info(rt_ctx* c, rt_denoise_info* out) { return c ? read_info(c, c->dn.info, out) : -1; }

int rt_denoise_variance(rt_ctx* c, const rt_vdenoise_params* params)
{
    return denoise_variance_call(c, { "rt_denoise_variance", "rt_multi_denoise_variance", "source 1, and " }, params);
}
int rt_read_variance(rt_ctx* c, float* var, size_t n) { return read_own(c, OwnPlane::Variance, var, n, false); }
int rt_copy_variance_to_device(rt_ctx* c, void* dst, size_t n) { return read_own(c, OwnPlane::Variance, dst, n, true); }
int rt_get_vdenoise_info(rt_ctx* c, rt_vdenoise_info* out) { return c ? read_info(c, c->vd.info, out) : -1; }

int rt_temporal(rt_ctx* c, const rt_temporal_params* params) { return temporal_call(c, { "rt_temporal", "rt_multi_temporal" }, params); }
int rt_denoise_temporal(rt_ctx* c, const rt_denoise_params* params)
{
    return denoise_call(c, { "rt_denoise_temporal", "rt_multi_temporal" }, true, params);
}
int rt_reset_temporal(rt_ctx* c)
{
    if (!c) return -1;
    RT_SETTLE(c);
    c->tp.reset();
    return 0;
}
int rt_read_temporal(rt_ctx* c, float* rgba, size_t n) { return read_own(c, OwnPlane::Temporal, rgba, n, false); }
int rt_read_temporal_history(rt_ctx* c, float* hist, size_t n) { return read_own(c, OwnPlane::History, hist, n, false); }
int rt_copy_temporal_to_device(rt_ctx* c, void* dst, size_t n) { return read_own(c, OwnPlane::Temporal, dst, n, true); }
int rt_read_temporal_display(rt_ctx* c, uint32_t* rgba8, size_t n_pixels)
{
    if (!c) return -1;
    RT_SETTLE(c);
    return read_filter_display(c, c, c->tp, "rt_temporal", c->tp.t[c->tp.cur].p, c->d_display, rgba8, n_pixels);
}
int rt_get_temporal_info(rt_ctx* c, rt_temporal_info* out) { return c ? read_info(c, c->tp.info, out) : -1; }

} // extern "C"
