"""The denoiser without a GPU: the checker (tests/denoise_oracle.c) is pinned to a float64 restatement of the definition and to analytic
cases, the definition is shown to reduce the error of a noisy render, and the ABI is declared, exported and bound.

(a) Float64 twin.  denoise_check.twin64 restates include/rt.h's text in float64 with exact 2**x.  Summation order and the polynomial's
    error are the only sources of difference.  Measured over the twelve cases below (37 x 23, demodulation on / off, 1 / 3 / 6
    iterations, two seeds each): largest absolute difference 3.8e-7 (values in [0, 1]), largest relative difference 4.9e-7 (on values
    >= 1e-3).  The bounds asserted are 4x those: 1.52e-6 and 1.96e-6.  Two deliberate misreadings (clamped borders, a colour sigma
    that does not halve) must fail the same comparison.
(b) A normal edge with sigmaNormal 0.1: x = 200 > 150, exp2_ is exactly 0, the halves filter as images of their own.
(c) One pass over white noise with a constant guide: the variance falls to (70/256)^2.
(d) mesh_test_scene at 96 x 64: denoised RMSE below noisy RMSE against a converged oracle image, defaults, 1 and 4 spp, both RNG modes.
(e) The boundary: symbols, struct sizes and field orders, the three host layers, the kernels' resources."""
import os
import re

import numpy as np
import pytest

import aov_check
import denoise_check
from test_camera_batch_cpu import built_library
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata

EXPORTS = ("rt_denoise", "rt_read_denoised", "rt_copy_denoised_to_device", "rt_read_denoised_display", "rt_get_denoise_info",
           "rt_multi_denoise", "rt_multi_read_denoised", "rt_multi_read_denoised_display")

# (a): measured largest differences over TWIN_CASES, and the asserted bounds = 4x
TWIN_MEASURED_ABS, TWIN_MEASURED_REL = 3.8e-7, 4.9e-7
TWIN_ABS, TWIN_REL = 4 * TWIN_MEASURED_ABS, 4 * TWIN_MEASURED_REL
TWIN_SIGMAS = dict(sigmaColour=0.5, sigmaNormal=0.25, sigmaDepth=0.1)
TWIN_CASES = [(demod, it, seed) for demod in (0, 1) for it in (1, 3, 6) for seed in (11, 12)]


def _twin_difference(got, want):
    """(largest absolute difference, largest relative difference on values >= 1e-3)"""
    got, want = got.astype(np.float64), want.astype(np.float64)
    diff = np.abs(got - want)
    big = np.abs(want) >= 1e-3
    return float(diff.max()), float((diff[big] / np.abs(want[big])).max())


@pytest.mark.parametrize("demod,iterations,seed", TWIN_CASES)
def test_checker_agrees_with_the_float64_twin(demod, iterations, seed):
    C, A, G = denoise_check.random_inputs(37, 23, seed)
    kw = dict(iterations=iterations, demodulate=demod, **TWIN_SIGMAS)
    got = denoise_check.checker(C, A, G, **kw)
    want = denoise_check.twin64(C, A, G, **kw)
    a, r = _twin_difference(got, want)
    print(f"demodulate {demod}, {iterations} iterations, seed {seed}: max abs {a:.3e}, max rel {r:.3e}")
    assert a <= TWIN_ABS and r <= TWIN_REL, (a, r)
    np.testing.assert_array_equal(got[..., 3], C[..., 3])


@pytest.mark.parametrize("variant,iterations", [(1, 1), (1, 3), (2, 3), (2, 6)])
def test_misreadings_of_the_definition_fail_the_twin_comparison(variant, iterations):
    """clamped borders (1) and a colour sigma that does not halve (2; it needs a second pass to show)"""
    C, A, G = denoise_check.random_inputs(37, 23, 11)
    kw = dict(iterations=iterations, demodulate=1, **TWIN_SIGMAS)
    a, r = _twin_difference(denoise_check.checker(C, A, G, variant=variant, **kw), denoise_check.twin64(C, A, G, **kw))
    assert a > 10 * TWIN_ABS and r > 10 * TWIN_REL, (a, r)


def test_exp2_copy_is_the_oracles(oracle):
    xs = np.concatenate([np.linspace(-151, 1, 4001), [-0.0, 0.0, -1e-8, -149.5, -150.0, -150.00002, -126.5, -127.49]]).astype(np.float32)
    for x in xs:
        a, b = denoise_check.shim().denoise_exp2(float(x)), oracle.lib.om_exp2(float(x))
        assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32), (x, a, b)


@pytest.mark.parametrize("demod,iterations", [(0, 1), (1, 4), (1, 6)])
def test_a_normal_edge_separates_the_image_exactly(demod, iterations):
    W, H = 40, 17
    C, A, G = denoise_check.random_inputs(W, H, 5)
    G[..., :3] = 0
    G[:, :W // 2, 0] = 1.0          # left: (1, 0, 0)
    G[:, W // 2:, 1] = 1.0          # right: (0, 1, 0): |dn|^2 = 2, x >= 2 / 0.01 = 200 > 150
    kw = dict(iterations=iterations, demodulate=demod, sigmaColour=1.0, sigmaNormal=0.1, sigmaDepth=0.5)
    whole = denoise_check.checker(C, A, G, **kw)
    for half in (slice(0, W // 2), slice(W // 2, W)):
        part = denoise_check.checker(C[:, half], A[:, half], G[:, half], **kw)
        aov_check.assert_same_bits(np.ascontiguousarray(whole[:, half]), part, f"half {half}")


def test_one_pass_over_white_noise_reduces_the_variance_by_the_kernels_sum_of_squares():
    """constant guide, sigmas 1e6: every weight is h[dy] * h[dx] (exp2_(-x) = 1 to within 1e-12), the output is a fixed linear filter of
    the input with sum(w^2) = (sum h^2)^2 = (70/256)^2.  Interior pixels (all 25 taps inside): n = 60 * 60 = 3600.  The sample variance
    of n correlated Gaussian outputs has relative standard error < sqrt(2 * K / n) with K = 25 the number of pixels an output is
    correlated with (5 x 5 overlapping supports weigh less than full correlation): sqrt(50 / 3600) = 0.118; bound = 4 sigma = 0.47."""
    W = H = 64
    rng = np.random.default_rng(2)
    C = np.zeros((H, W, 4), np.float32)
    C[..., :3] = rng.normal(0.0, 1.0, (H, W, 3)).astype(np.float32)
    A = np.ones((H, W, 4), np.float32)
    G = np.zeros((H, W, 4), np.float32)
    G[..., 1], G[..., 3] = 1.0, 5.0
    out = denoise_check.checker(C, A, G, iterations=1, demodulate=0, sigmaColour=1e6, sigmaNormal=1e6, sigmaDepth=1e6)
    n = 60 * 60
    bound = 4 * np.sqrt(2 * 25 / n)
    want = (70 / 256) ** 2
    for ch in range(3):
        ratio = out[2:-2, 2:-2, ch].astype(np.float64).var() / C[2:-2, 2:-2, ch].astype(np.float64).var()
        print(f"channel {ch}: variance ratio {ratio:.5f}, want {want:.5f} within {bound:.2f} relative")
        assert abs(ratio / want - 1) < bound, (ch, ratio, want)


# ---- (d) quality of the definition -------------------------------------------------------------------------------------------------
QW, QH = 96, 64


def _scene(rtx, spp, mode):
    params, spheres, tris, infos = rtx.scenes.mesh_test_scene(QW, QH).build_buffers()
    params["numRaysPerPixel"], params["rngMode"] = spp, mode
    return params, spheres, tris, infos


@pytest.fixture(scope="module")
def converged(rtx, oracle):
    """the same scene, 8 frames of 128 samples per pixel = 1024 in total (frame indices away from the noisy frames')"""
    p, s, t, m = _scene(rtx, 128, 1)
    image = oracle.render(p, s, t, m, 1000, 8, accel=True)[0]
    image.setflags(write=False)
    return image


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_denoised_image_is_closer_to_the_converged_image_than_the_noisy_one(rtx, oracle, converged, spp, mode):
    p, s, t, m = _scene(rtx, spp, mode)
    noisy = oracle.render(p, s, t, m, 0, 1, accel=True)[0]
    A, G = aov_check.oracle_planes(rtx, p, s, t, m, range(4))
    den = denoise_check.checker(noisy, A, G, **denoise_check.DEFAULTS)
    before, after = denoise_check.rmse(noisy, converged), denoise_check.rmse(den, converged)
    print(f"{spp} spp, rngMode {mode}: RMSE noisy {before:.4f}, denoised {after:.4f}, ratio {after / before:.3f}")
    assert after < before


# ---- (e) the boundary ----------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt.h")).read(), flags=re.S)


def _c_fields(header, name):
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", header, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(?:const\s+)?\w+\s+", "", decl.strip())
        if decl:
            names += [re.sub(r"\[.*?\]", "", d).strip() for d in decl.split(",")]
    return names


def test_entry_points_are_declared_exported_and_bound(rtx):
    header = _header()
    lib = rtx.load_library()
    for name in EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in rtx._cabi.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    for cls in (rtx.Tracer, rtx.MultiTracer):
        for method in ("denoise", "read_denoised", "read_denoised_display", "denoise_info"):
            assert hasattr(cls, method), (cls.__name__, method)
    assert hasattr(rtx.RayTracingManager, "Denoise")
    assert lib.rt_abi_version() == 1
    assert lib.rt_sizeof(b"rt_denoise_params") == 32 == rtx.DENOISE_PARAMS.itemsize
    assert lib.rt_sizeof(b"rt_denoise_info") == 32 == rtx.DENOISE_INFO.itemsize
    assert _c_fields(header, "rt_denoise_params") == list(rtx.DENOISE_PARAMS.names)
    assert _c_fields(header, "rt_denoise_info") == list(rtx.DENOISE_INFO.names)
    # the defaults of the header, of the binding and of the tests' checker are the same
    for key, macro in (("iterations", "ITERATIONS"), ("demodulate", "DEMODULATE"), ("sigmaColour", "SIGMA_COLOUR"),
                       ("sigmaNormal", "SIGMA_NORMAL"), ("sigmaDepth", "SIGMA_DEPTH")):
        value = float(re.search(r"#define\s+RT_DENOISE_DEFAULT_" + macro + r"\s+([\d.]+)f?", header).group(1))
        assert value == rtx.DENOISE_DEFAULTS[key] == denoise_check.DEFAULTS[key], key


def test_csharp_and_cpp_hosts_carry_the_denoiser():
    cs = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cs")
    native, backend = open(os.path.join(cs, "RtNative.cs")).read(), open(os.path.join(cs, "RtBackend.cs")).read()
    for name in EXPORTS:
        assert re.search(r"static\s+extern\s+int\s+" + name + r"\s*\(", native), name
    used = set(re.findall(r"RtNative\.(\w+)", backend))
    for name in ("rt_denoise", "rt_read_denoised", "rt_multi_denoise", "rt_multi_read_denoised"):
        assert name in used, name
    text = open(os.path.join(cs, "RtDenoise.cs")).read()
    structs = dict(re.findall(r"public\s+struct\s+(\w+)[^{]*\{(.*?)\n    \}", text, re.S))
    fields = {k: re.findall(r"public\s+(int|float|double)\s+([\w, ]+);", v) for k, v in structs.items()}
    flat = {k: [(t, n.strip()) for t, names in v for n in names.split(",")] for k, v in fields.items()}
    assert flat["RtDenoiseParams"] == [("int", "iterations"), ("int", "demodulate"), ("float", "sigmaColour"), ("float", "sigmaNormal"),
                                       ("float", "sigmaDepth"), ("int", "_reserved0"), ("int", "_reserved1"), ("int", "_reserved2")]
    assert flat["RtDenoiseInfo"] == [("int", "iterations"), ("int", "demodulate"), ("int", "width"), ("int", "height"),
                                     ("double", "lastKernelMs"), ("double", "totalKernelMs")]
    hpp = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp", "rt_host.hpp")).read()
    cpp = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp", "rt_host.cpp")).read()
    assert re.search(r"\bDenoise\s*\(", hpp) and re.search(r"\brt_denoise\b", cpp) and re.search(r"\brt_multi_denoise\b", cpp)


def test_denoise_kernels_are_built_without_scratch_or_spilled_vgprs():
    passes, preps = set(), set()
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            name = k[".name"]
            if "k_atrous" in name or "k_denoise" in name:
                (passes if "k_atrous" in name else preps).add(name)
                assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, (name, "scratch")
                assert not any(s in name for s in ("k_aov", "k_trace", "k_stream")), name
    assert len(passes) == 2 and len(preps) == 1, (sorted(passes), sorted(preps))        # k_atrous<false / true>, k_denoise_prep
