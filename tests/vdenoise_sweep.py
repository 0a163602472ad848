"""The sweep behind the variance-guided denoiser's defaults (RT_VDENOISE_DEFAULT_* of include/rt.h): on mesh_test_scene at 96 x 64, the
RMSE of the checker's image against a converged oracle image (8 frames of 128 samples per pixel, frame k blended with weight 1 / (k + 1)
from k = 0, as tests/test_temporal_cpu.py builds its own), over sigmaLuminance x sigmaNormal x sigmaDepth x demodulate x iterations, for 1
and 4 samples per pixel in both RNG modes.  The score of a grid point is the mean over the four cases of RMSE(filtered) / RMSE(noisy);
the best point becomes the defaults.  The same grid of rt_denoise's checker (sigmaColour in place of sigmaLuminance) is swept beside it,
for comparison only.  Writes the table to profiles/vdenoise_defaults.txt.

    python tests/vdenoise_sweep.py            (CPU only: the oracle and the two checkers)"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import aov_check            # noqa: E402
import denoise_check        # noqa: E402
import oracle_binding       # noqa: E402
import rtx_pkg              # noqa: E402
import vdenoise_check       # noqa: E402

W, H = 96, 64
CONVERGED_SPP, CONVERGED_FRAMES = 128, 8
FEATURE_FRAMES = 4
SIGMA_L = (1.0, 2.0, 4.0, 8.0, 16.0)
SIGMA_C = (0.25, 0.5, 1.0, 2.0, 4.0, 16.0)
SIGMA_N = (0.1, 0.25, 0.5, 1.0)
SIGMA_D = (0.02, 0.1, 0.5, 2.0)
ITERATIONS = (3, 4, 5)


def scene(rtx, spp, rng_mode):
    params, spheres, tris, infos = rtx.scenes.mesh_test_scene(W, H).build_buffers()
    params["numRaysPerPixel"], params["rngMode"] = spp, rng_mode
    return params, spheres, tris, infos


def converged_image(rtx, orc):
    """CONVERGED_FRAMES frames of CONVERGED_SPP samples (Philox, frame indices away from the noisy frames'), the running mean from k = 0"""
    p, s, t, m = scene(rtx, CONVERGED_SPP, 1)
    image = None
    for k in range(CONVERGED_FRAMES):
        cur = orc.render_frame(p, s, t, m, 1000 + k, accel=True)[0]
        image = np.zeros_like(cur) if image is None else image
        orc.accumulate(image, cur, k)
    return image


def noisy_case(rtx, orc, spp, mode):
    """(resultTexture after one frame, the feature planes of FEATURE_FRAMES frames)"""
    p, s, t, m = scene(rtx, spp, mode)
    cur = orc.render_frame(p, s, t, m, 0, accel=True)[0]
    noisy = np.zeros_like(cur)
    orc.accumulate(noisy, cur, 0)
    A, G = aov_check.oracle_planes(rtx, p, s, t, m, range(FEATURE_FRAMES))
    return noisy, A, G


def cases(rtx, orc):
    out = []
    for spp in (1, 4):
        for mode in (0, 1):
            out.append((f"{spp} spp, {'Philox' if mode else 'PCG'}",) + noisy_case(rtx, orc, spp, mode))
    return out


def main():
    rtx = rtx_pkg.load()
    orc = oracle_binding.Oracle()
    converged, cs = converged_image(rtx, orc), cases(rtx, orc)
    noisy_rmse = [denoise_check.rmse(c[1], converged) for c in cs]

    def sweep(filter_image, sigmas):
        rows = []
        for demod, it, s0, sn, sd in itertools.product((0, 1), ITERATIONS, sigmas, SIGMA_N, SIGMA_D):
            rm = [denoise_check.rmse(filter_image(noisy, A, G, it, demod, s0, sn, sd), converged) for _, noisy, A, G in cs]
            rows.append((float(np.mean([r / n for r, n in zip(rm, noisy_rmse)])), demod, it, s0, sn, sd, rm))
        rows.sort(key=lambda r: r[0])
        return rows
    vrows = sweep(lambda *a: vdenoise_check.checker(*a)[0], SIGMA_L)
    drows = sweep(denoise_check.checker, SIGMA_C)
    dflt = [denoise_check.rmse(denoise_check.checker(noisy, A, G, **denoise_check.DEFAULTS), converged) for _, noisy, A, G in cs]
    head = " | ".join(c[0] for c in cs)
    fmt = lambda r: f"{r[0]:.4f}  {r[1]:10d} {r[2]:10d} {r[3]:9.2f} {r[4]:11.2f} {r[5]:10.2f} | " + " | ".join(f"{x:.4f}" for x in r[6])   # noqa: E731
    lines = [f"Variance-guided denoiser defaults: sweep on mesh_test_scene {W}x{H}, {FEATURE_FRAMES} feature frames, against a converged oracle",
             f"image ({CONVERGED_FRAMES} frames of {CONVERGED_SPP} samples per pixel, Philox mode, frame k weighted 1 / (k + 1) from k = 0).  CPU: oracle +",
             "tests/vdenoise_oracle.c (and tests/denoise_oracle.c for the comparison).  score = mean over the four cases of",
             "RMSE(filtered) / RMSE(noisy); the columns of the cases hold the RMSE itself; sorted by score, the first row is the default.",
             "",
             "noisy RMSE:                        " + ", ".join(f"{c[0]}: {r:.4f}" for c, r in zip(cs, noisy_rmse)),
             "rt_denoise at RT_DENOISE_DEFAULT_*: " + ", ".join(f"{c[0]}: {r:.4f}" for c, r in zip(cs, dflt)),
             "",
             "rt_denoise_variance",
             "score   demodulate iterations  sigmaLum sigmaNormal sigmaDepth | " + head]
    lines += [fmt(r) for r in vrows]
    lines += ["", "rt_denoise (fixed colour sigma), the same grid: for comparison only",
              "score   demodulate iterations  sigmaCol sigmaNormal sigmaDepth | " + head]
    lines += [fmt(r) for r in drows]
    with open(os.path.join(ROOT, "profiles", "vdenoise_defaults.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:22]))
    print("\n".join(lines[len(vrows) + 10:len(vrows) + 18]))


if __name__ == "__main__":
    main()
