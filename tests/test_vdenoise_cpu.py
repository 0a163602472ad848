"""The variance-guided denoiser without a GPU: the checker (tests/vdenoise_oracle.c) is pinned to a float64 restatement of the definition
and to analytic cases, the estimator and the propagated variance are checked against their expectations, the variance is shown to buy an
edge rt_denoise loses and a lower error on a noisy render, and the ABI is declared, exported and bound.

(a) Float64 twin.  vdenoise_check.twin64 restates include/rt.h's text in float64 with exact 2**x.  Summation order and the polynomial's
    error are the only sources of difference.  Measured over the twelve cases below (37 x 23, demodulation on / off, 1 / 2 / 5
    iterations, colour_max 1 and 1e4): largest absolute difference of the image 1.7e-6 of colour_max (demodulated values reach 100 times
    colour_max), largest relative difference 1.8e-6 (on values >= 1e-3 of colour_max), largest difference of var_0 2.4e-6 of its largest
    value.  The bounds asserted are 4x those: 6.8e-6, 7.2e-6 and 9.6e-6.  Three deliberate misreadings (clamped borders, the prefilter
    at spacing s, variance weighted by w) must fail the same comparison by more than 10x (measured: 0.4 and more).
(b) Exact cases: a constant image, images smaller than the windows, strips, a normal edge with disjoint geometry weights.
(c) The estimator on white noise: mean var_0 = sigma^2 * 48/49; one pass from a constant variance: var * (70/256)^2.
(d) A luminance step of 20 sigma: kept by the variance-guided filter, lost by rt_denoise at its defaults.
(e) mesh_test_scene at 96 x 64: RMSE below the noisy image's and below rt_denoise's at its defaults, 1 and 4 spp, both RNG modes.
(f) The boundary: symbols, struct sizes and field orders, the three host layers, the kernels' resources."""
import os
import re

import numpy as np
import pytest

import aov_check
import denoise_check
import vdenoise_check
import vdenoise_sweep
from test_camera_batch_cpu import built_library
from test_denoise_cpu import _c_fields, _header
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata

EXPORTS = ("rt_denoise_variance", "rt_read_variance", "rt_copy_variance_to_device", "rt_get_vdenoise_info",
           "rt_multi_denoise_variance", "rt_multi_read_variance")

# (a): measured largest differences over TWIN_CASES (image: absolute / colour_max, and relative on values >= 1e-3 * colour_max; var_0:
# relative to its largest value), and the asserted bounds = 4x
TWIN_MEASURED_ABS, TWIN_MEASURED_REL, TWIN_MEASURED_VAR = 1.7e-6, 1.8e-6, 2.4e-6
TWIN_ABS, TWIN_REL, TWIN_VAR = 4 * TWIN_MEASURED_ABS, 4 * TWIN_MEASURED_REL, 4 * TWIN_MEASURED_VAR
TWIN_SIGMAS = dict(sigmaLuminance=2.0, sigmaNormal=0.25, sigmaDepth=0.1)
TWIN_CASES = [(demod, it, cmax) for demod in (0, 1) for it in (1, 2, 5) for cmax in (1.0, 1e4)]


def _twin_difference(got, want, scale):
    """(largest absolute difference / scale, largest relative difference on values >= 1e-3 * scale)"""
    got, want = got.astype(np.float64), want.astype(np.float64)
    diff = np.abs(got - want)
    big = np.abs(want) >= 1e-3 * scale
    return float(diff.max()) / scale, float((diff[big] / np.abs(want[big])).max())


def _twin_case(W, H, seed, cmax, variant=0, **kw):
    """(abs, rel, var): the checker's differences from the twin on random inputs"""
    C, A, G = vdenoise_check.random_inputs(W, H, seed, colour_max=cmax)
    got, got_var = vdenoise_check.checker(C, A, G, variant=variant, **kw)
    want, want_var = vdenoise_check.twin64(C, A, G, **kw)
    np.testing.assert_array_equal(got[..., 3], C[..., 3])
    a, r = _twin_difference(got[..., :3], want[..., :3], cmax)
    v = float(np.abs(got_var.astype(np.float64) - want_var).max() / want_var.max())
    return a, r, v


@pytest.mark.parametrize("demod,iterations,cmax", TWIN_CASES)
def test_checker_agrees_with_the_float64_twin(demod, iterations, cmax):
    a, r, v = _twin_case(37, 23, 11 + iterations, cmax, iterations=iterations, demodulate=demod, **TWIN_SIGMAS)
    print(f"demodulate {demod}, {iterations} iterations, colour_max {cmax:g}: max abs {a:.3e}, max rel {r:.3e}, var_0 {v:.3e}")
    assert a <= TWIN_ABS and r <= TWIN_REL and v <= TWIN_VAR, (a, r, v)


@pytest.mark.parametrize("variant,iterations", [(1, 1), (1, 5), (2, 2), (2, 5), (3, 2), (3, 5)])
def test_misreadings_of_the_definition_fail_the_twin_comparison(variant, iterations):
    """clamped borders (1), the prefilter at spacing s (2) and variance weighted by w (3); 2 and 3 need a second pass to show: pass 0 has
    s = 1, and var_1 is first read by pass 1"""
    a, r, _ = _twin_case(37, 23, 11, 1.0, variant=variant, iterations=iterations, demodulate=1, **TWIN_SIGMAS)
    assert a > 10 * TWIN_ABS and r > 10 * TWIN_REL, (a, r)


def test_exp2_copy_is_the_oracles(oracle):
    xs = np.concatenate([np.linspace(-151, 1, 4001), [-0.0, 0.0, -1e-8, -149.5, -150.0, -150.00002, -126.5, -127.49]]).astype(np.float32)
    for x in xs:
        a, b = vdenoise_check.shim().vdenoise_exp2(float(x)), oracle.lib.om_exp2(float(x))
        assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32), (x, a, b)


# ---- (b) exact cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demod", [0, 1])
def test_a_constant_image_has_no_variance_and_comes_back_bit_for_bit(demod):
    """every luminance is equal: m2 / sg - mu * mu is 0.25 - 0.25 (0.5 and its square are exact, and sum(g * c) / sum(g) = c exactly when
    every product g * 0.5 is a halving), so var_0 = 0, kl = 1e6, every luminance difference is 0 and a pass is a mean of equal values.
    With demodulation the albedo is constant too, so e0 is constant and out = e0 * d = C to rounding of one quotient and one product."""
    W, H = 37, 23
    _, A, G = vdenoise_check.random_inputs(W, H, 4)
    C = np.full((H, W, 4), 0.5, np.float32)
    if demod:
        A[..., :3], A[..., 3] = 0.5, 1.0            # d = 0.5: e0 = 1.0, out = 1.0 * 0.5
    out, var = vdenoise_check.checker(C, A, G, **dict(vdenoise_check.DEFAULTS, demodulate=demod))
    assert (var == 0).all()
    aov_check.assert_same_bits(out, C, "a constant image")


@pytest.mark.parametrize("w,h", [(3, 2), (1, 40), (40, 1)])
def test_images_smaller_than_the_windows_agree_with_the_twin(w, h):
    for iterations in (1, 5):
        a, r, v = _twin_case(w, h, 9, 1.0, iterations=iterations, demodulate=1, **TWIN_SIGMAS)
        print(f"{w} x {h}, {iterations} iterations: max abs {a:.3e}, max rel {r:.3e}, var_0 {v:.3e}")
        assert a <= TWIN_ABS and r <= TWIN_REL and v <= TWIN_VAR, (a, r, v)


@pytest.mark.parametrize("demod,iterations,reach", [(0, 1, 1), (1, 2, 5), (1, 3, 13)])
def test_a_normal_edge_separates_the_image_exactly(demod, iterations, reach):
    """Across the edge |dn|^2 = 2 and x >= 2 / 0.01 = 200 > 150, so g and w are exactly 0: var_0 of each half is that of the half as an
    image of its own, bit for bit, and so is the filtered image outside the reach of the prefilter.  The 3 x 3 prefilter has no
    geometry weight (the definition gives it none), so gv of the column next to the edge reads var_i across it, where the half on its
    own has an image border: that column's kl differs, and each later pass carries the difference 2 s further.  Columns nearer to the
    edge than `reach` = 1, 1 + 4, 1 + 4 + 8 are left out; every other pixel is exact."""
    W, H = 64, 17
    C, A, G = vdenoise_check.random_inputs(W, H, 5)
    G[..., :3] = 0
    G[:, :W // 2, 0] = 1.0          # left: (1, 0, 0)
    G[:, W // 2:, 1] = 1.0          # right: (0, 1, 0)
    kw = dict(iterations=iterations, demodulate=demod, sigmaLuminance=4.0, sigmaNormal=0.1, sigmaDepth=0.5)
    whole, whole_var = vdenoise_check.checker(C, A, G, **kw)
    for half, far in ((slice(0, W // 2), slice(0, W // 2 - reach)), (slice(W // 2, W), slice(reach, W // 2))):
        part, part_var = vdenoise_check.checker(C[:, half], A[:, half], G[:, half], **kw)
        aov_check.assert_same_bits(np.ascontiguousarray(whole_var[:, half])[..., None], part_var[..., None], f"half {half}: var_0")
        aov_check.assert_same_bits(np.ascontiguousarray(whole[:, half][:, far]), np.ascontiguousarray(part[:, far]), f"half {half}")
        np.testing.assert_array_equal(whole[:, half][..., 3], part[..., 3])


# ---- (c) the estimator and the propagated variance ------------------------------------------------------------------------------------
def _flat_guides(W, H):
    A = np.ones((H, W, 4), np.float32)
    G = np.zeros((H, W, 4), np.float32)
    G[..., 1], G[..., 3] = 1.0, 5.0
    return A, G


def test_the_estimate_of_white_noise_is_its_variance():
    """128 x 128, constant geometry (every g = 1), grey noise of standard deviation sigma on a constant colour: var_0 is the biased sample
    variance of 49 values, expectation sigma^2 * 48/49.  Each estimate has relative standard deviation sqrt(2/48) = 0.20; the interior
    (122 x 122) holds about 300 disjoint windows, so the mean's standard error is about 1.2 %; 5 % is 4 standard errors."""
    W = H = 128
    sigma = 0.05
    rng = np.random.default_rng(6)
    C = np.ones((H, W, 4), np.float32)
    C[..., :3] = (0.5 + rng.normal(0.0, sigma, (H, W, 1))).astype(np.float32)
    A, G = _flat_guides(W, H)
    var = vdenoise_check.checker_variance(C, A, G)
    mean, want = float(var[3:-3, 3:-3].astype(np.float64).mean()), sigma * sigma * 48 / 49
    print(f"mean var_0 {mean:.6e}, want {want:.6e}, ratio {mean / want:.4f}")
    assert abs(mean / want - 1) < 0.05


def test_one_pass_carries_a_constant_variance_by_the_kernels_sum_of_squares():
    """constant guide and constant colour, sigmaLuminance 1e6: every weight is h[dy] * h[dx] exactly, so interior pixels (all 25 taps
    inside) have var_1 = var_0 * sum(w^2) / sum(w)^2 = var_0 * (70/256)^2 with sum(w) = 1: 25 products, 25 sums and one quotient, each
    within half an ulp: 2^-24 * 51 < 4e-6 relative."""
    W = H = 24
    _, G = _flat_guides(W, H)
    e = np.full((H, W, 3), 0.25, np.float32)
    var = np.full((H, W), 0.37, np.float32)
    e2, var2 = vdenoise_check.checker_pass(e, var, G, step=2, sigmaLuminance=1e6)
    want = float(np.float32(0.37)) * (70 / 256) ** 2
    inner = var2[4:-4, 4:-4].astype(np.float64)
    assert np.abs(inner / want - 1).max() < 4e-6, (inner.min(), inner.max(), want)
    assert (var2[0, 0] > want * 1.5)                    # (a corner has 9 taps: fewer, heavier weights)
    np.testing.assert_array_equal(e2, e)


# ---- (d) what variance buys -----------------------------------------------------------------------------------------------------------
STEP_SIGMA, STEP_W, STEP_H = 0.02, 16384, 8


def test_a_luminance_step_is_kept_where_rt_denoise_loses_it():
    """Two flat halves 20 sigma apart, constant geometry, noise sigma on both; 5 passes at the default sigmas.
    The size: within 3 columns of the step the 7 x 7 estimate spans both levels, var_0 there is of the order of (10 sigma)^2 and the
    edge-stop is open, so a few columns at the step are smeared (this is the spatial estimate's known cost).  A smeared pixel stays
    between the two levels, so in a symmetric blur it leaves its own level by at most half the step, 10 sigma; counting the 3 columns
    of the estimate's reach and 2 more for the first pass's reach into them, a half's variance gains at most 5 * (10 sigma)^2 / (W / 2).
    At W = 16384 that is 0.061 sigma^2, which leaves the flat part (residual about (70/256)^2 per pass: < 0.01 sigma^2) room below
    sigma^2 / 10; the same count bounds the loss of the step between the halves' means by 2 * 5 * 10 sigma / (W / 2) = 0.06 % of it.
    rt_denoise at RT_DENOISE_DEFAULT_* (every colour weight 1: a geometry blur) on the same input loses more than half of the step
    between the two columns next to it."""
    W, H, sigma = STEP_W, STEP_H, STEP_SIGMA
    rng = np.random.default_rng(3)
    level = np.where(np.arange(W) < W // 2, 0.3, 0.3 + 20 * sigma)
    C = np.ones((H, W, 4), np.float32)
    C[..., :3] = (level[None, :, None] + rng.normal(0.0, sigma, (H, W, 1))).astype(np.float32)
    A, G = _flat_guides(W, H)
    out, _ = vdenoise_check.checker(C, A, G, **dict(vdenoise_check.DEFAULTS, iterations=5))
    left, right = out[:, :W // 2, 1].astype(np.float64), out[:, W // 2:, 1].astype(np.float64)
    step = (right.mean() - left.mean()) / (20 * sigma)
    vl, vr = left.var() / sigma ** 2, right.var() / sigma ** 2
    ref = denoise_check.checker(C, A, G, **denoise_check.DEFAULTS)
    ref_edge = float(ref[:, W // 2, 1].astype(np.float64).mean() - ref[:, W // 2 - 1, 1].astype(np.float64).mean()) / (20 * sigma)
    edge = float(out[:, W // 2, 1].astype(np.float64).mean() - out[:, W // 2 - 1, 1].astype(np.float64).mean()) / (20 * sigma)
    print(f"step kept {step:.5f}; variance / sigma^2 left {vl:.4f} right {vr:.4f}; step between the edge columns: variance-guided {edge:.3f}, "
          f"rt_denoise {ref_edge:.3f}")
    assert abs(step - 1) < 0.02
    assert vl < 0.1 and vr < 0.1
    assert ref_edge < 0.5


# ---- (e) quality of the definition ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def converged(rtx, oracle):
    image = vdenoise_sweep.converged_image(rtx, oracle)
    image.setflags(write=False)
    return image


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_variance_guided_image_beats_the_noisy_one_and_rt_denoise_at_its_defaults(rtx, oracle, converged, spp, mode):
    noisy, A, G = vdenoise_sweep.noisy_case(rtx, oracle, spp, mode)
    var_guided = vdenoise_check.checker(noisy, A, G, **vdenoise_check.DEFAULTS)[0]
    fixed = denoise_check.checker(noisy, A, G, **denoise_check.DEFAULTS)
    r = {k: denoise_check.rmse(v, converged) for k, v in (("noisy", noisy), ("variance-guided", var_guided), ("rt_denoise", fixed))}
    print(f"{spp} spp, rngMode {mode}: RMSE " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert r["variance-guided"] < r["noisy"]
    assert r["variance-guided"] < r["rt_denoise"]


# ---- (f) the boundary ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(rtx):
    header = _header()
    lib = rtx.load_library()
    for name in EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in rtx._cabi.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    for cls in (rtx.Tracer, rtx.MultiTracer):
        for method in ("denoise_variance", "read_variance"):
            assert hasattr(cls, method), (cls.__name__, method)
    assert hasattr(rtx.Tracer, "vdenoise_info") and hasattr(rtx.Tracer, "copy_variance_to_device")
    assert hasattr(rtx.RayTracingManager, "DenoiseVariance")
    assert lib.rt_abi_version() == 1
    assert lib.rt_sizeof(b"rt_vdenoise_params") == 32 == rtx.VDENOISE_PARAMS.itemsize
    assert lib.rt_sizeof(b"rt_vdenoise_info") == 32 == rtx.VDENOISE_INFO.itemsize
    assert _c_fields(header, "rt_vdenoise_params") == list(rtx.VDENOISE_PARAMS.names)
    assert _c_fields(header, "rt_vdenoise_info") == list(rtx.VDENOISE_INFO.names)
    # the defaults of the header, of the binding and of the tests' checker are the same
    for key, macro in (("iterations", "ITERATIONS"), ("demodulate", "DEMODULATE"), ("sigmaLuminance", "SIGMA_LUMINANCE"),
                       ("sigmaNormal", "SIGMA_NORMAL"), ("sigmaDepth", "SIGMA_DEPTH")):
        value = float(re.search(r"#define\s+RT_VDENOISE_DEFAULT_" + macro + r"\s+([\d.]+)f?", header).group(1))
        assert value == rtx.VDENOISE_DEFAULTS[key] == vdenoise_check.DEFAULTS[key], key
    assert rtx.VDENOISE_DEFAULTS["source"] == 0


def test_csharp_and_cpp_hosts_carry_the_variance_guided_denoiser():
    cs = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cs")
    native, backend = open(os.path.join(cs, "RtNative.cs")).read(), open(os.path.join(cs, "RtBackend.cs")).read()
    for name in EXPORTS:
        assert re.search(r"static\s+extern\s+int\s+" + name + r"\s*\(", native), name
    used = set(re.findall(r"RtNative\.(\w+)", backend))
    for name in ("rt_denoise_variance", "rt_read_variance", "rt_multi_denoise_variance", "rt_multi_read_variance"):
        assert name in used, name
    text = open(os.path.join(cs, "RtDenoise.cs")).read()
    structs = dict(re.findall(r"public\s+struct\s+(\w+)[^{]*\{(.*?)\n    \}", text, re.S))
    fields = {k: re.findall(r"public\s+(int|float|double)\s+([\w, ]+);", v) for k, v in structs.items()}
    flat = {k: [(t, n.strip()) for t, names in v for n in names.split(",")] for k, v in fields.items()}
    assert flat["RtVDenoiseParams"] == [("int", "iterations"), ("int", "demodulate"), ("int", "source"), ("float", "sigmaLuminance"),
                                        ("float", "sigmaNormal"), ("float", "sigmaDepth"), ("int", "_reserved0"), ("int", "_reserved1")]
    assert flat["RtVDenoiseInfo"] == [("int", "iterations"), ("int", "source"), ("int", "width"), ("int", "height"),
                                      ("double", "lastKernelMs"), ("double", "totalKernelMs")]
    hpp = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp", "rt_host.hpp")).read()
    cpp = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp", "rt_host.cpp")).read()
    assert re.search(r"\bDenoiseVariance\s*\(", hpp) and re.search(r"\brt_denoise_variance\b", cpp) and re.search(r"\brt_multi_denoise_variance\b", cpp)


def test_variance_kernels_are_built_without_scratch_or_spilled_vgprs():
    passes, estimates = set(), set()
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            name = k[".name"]
            if "k_var_atrous" in name or "k_variance_estimate" in name:
                (passes if "k_var_atrous" in name else estimates).add(name)
                assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, (name, "scratch")
    assert len(passes) == 2 and len(estimates) == 1, (sorted(passes), sorted(estimates))    # k_var_atrous<false / true>, k_variance_estimate
