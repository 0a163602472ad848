"""The sweep behind the denoiser's defaults (RT_DENOISE_DEFAULT_* of include/rt.h): on mesh_test_scene at 96 x 64, the RMSE of the
checker's denoised image against a converged oracle image (1024 samples per pixel), over a small grid of the three sigmas and the
demodulation switch, for 1 and 4 samples per pixel in both RNG modes.  The score of a grid point is the mean over the four cases of
RMSE(denoised) / RMSE(noisy); the best point becomes the defaults.  Writes the table to profiles/denoise_defaults.txt.

    python tests/denoise_sweep.py            (CPU only: the oracle and the checker)"""
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

W, H = 96, 64
CONVERGED_SPP, CONVERGED_FRAMES = 128, 8
FEATURE_FRAMES = 4
ITERATIONS = 5


def scene(rtx, spp, rng_mode):
    mgr = rtx.scenes.mesh_test_scene(W, H)
    params, spheres, tris, infos = mgr.build_buffers()
    params["numRaysPerPixel"], params["rngMode"] = spp, rng_mode
    return params, spheres, tris, infos


def cases(rtx, orc):
    """(converged image, [(label, noisy image, albedo plane, normal-depth plane)])"""
    p, s, t, m = scene(rtx, CONVERGED_SPP, 1)
    converged = orc.render(p, s, t, m, 1000, CONVERGED_FRAMES, accel=True)[0]
    out = []
    for spp in (1, 4):
        for mode in (0, 1):
            p, s, t, m = scene(rtx, spp, mode)
            noisy = orc.render(p, s, t, m, 0, 1, accel=True)[0]
            A, G = aov_check.oracle_planes(rtx, p, s, t, m, range(FEATURE_FRAMES))
            out.append((f"{spp} spp, {'Philox' if mode else 'PCG'}", noisy, A, G))
    return converged, out


def main():
    rtx = rtx_pkg.load()
    orc = oracle_binding.Oracle()
    converged, cs = cases(rtx, orc)
    noisy_rmse = [denoise_check.rmse(c[1], converged) for c in cs]
    grid = list(itertools.product((0, 1), (0.5, 1.0, 2.0, 4.0, 8.0, 16.0), (0.1, 0.25, 0.5, 1.0), (0.02, 0.1, 0.5, 2.0)))
    rows = []
    for demod, sc, sn, sd in grid:
        ratios = []
        for (label, noisy, A, G), nr in zip(cs, noisy_rmse):
            den = denoise_check.checker(noisy, A, G, ITERATIONS, demod, sc, sn, sd)
            ratios.append(denoise_check.rmse(den, converged) / nr)
        rows.append((float(np.mean(ratios)), demod, sc, sn, sd, ratios))
    rows.sort(key=lambda r: r[0])
    lines = [f"Denoiser defaults: sweep on mesh_test_scene {W}x{H}, {ITERATIONS} iterations, {FEATURE_FRAMES} feature frames,",
             f"against a converged oracle image ({CONVERGED_SPP * CONVERGED_FRAMES} samples per pixel, Philox mode).  CPU: oracle + tests/denoise_oracle.c.",
             "ratio = RMSE(denoised) / RMSE(noisy); score = mean of the four ratios; sorted by score, the first row is the default.",
             "",
             "noisy RMSE: " + ", ".join(f"{c[0]}: {r:.4f}" for c, r in zip(cs, noisy_rmse)),
             "",
             "score   demodulate sigmaColour sigmaNormal sigmaDepth | " + " | ".join(c[0] for c in cs)]
    for score, demod, sc, sn, sd, ratios in rows:
        lines.append(f"{score:.4f}  {demod:10d} {sc:11.2f} {sn:11.2f} {sd:10.2f} | " + " | ".join(f"{r:.4f}" for r in ratios))
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "denoise_defaults.txt"), "w") as f:
        f.write(text)
    print("\n".join(lines[:12]))


if __name__ == "__main__":
    main()
