"""The sweep behind the defaults of temporal reprojection (RT_TEMPORAL_DEFAULT_* of include/rt.h): the set-up of the quality test of
tests/test_temporal_cpu.py (mesh_test_scene at 96 x 64, a path of 8 poses with one frame each, 1 and 4 samples per pixel in both RNG
modes, against a converged oracle image of the last pose), over a small grid of maxHistory and the two tolerances.  The score of a grid
point is the mean over the four cases of RMSE(T) / RMSE(single frame) at the last pose; the best point becomes the defaults.  Writes the
table to profiles/temporal_defaults.txt.

    python tests/temporal_sweep.py            (CPU only: the oracle and the checkers)"""
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
import temporal_check       # noqa: E402
import test_temporal_cpu as q       # noqa: E402


def main():
    rtx = rtx_pkg.load()
    orc = oracle_binding.Oracle()
    poses, s, t, m = q.path_params(rtx, 128, 1)
    converged = None
    for k in range(8):
        cur = orc.render_frame(poses[-1], s, t, m, 1000 + k, accel=True)[0]
        converged = np.zeros_like(cur) if converged is None else converged
        orc.accumulate(converged, cur, k)
    poses4, s, t, m = q.path_params(rtx, 4, 1)
    guides = [aov_check.oracle_planes(rtx, p, s, t, m, range(4)) for p in poses4]
    cases = []
    for spp in (1, 4):
        for mode in (0, 1):
            poses, s, t, m = q.path_params(rtx, spp, mode)
            frames, accum = [], None
            for i, p in enumerate(poses):
                cur = orc.render_frame(p, s, t, m, i, accel=True)[0]
                frame = np.zeros_like(cur)
                orc.accumulate(frame, cur, 0)
                accum = np.zeros_like(cur) if accum is None else accum
                orc.accumulate(accum, cur, i)
                frames.append(frame)
            cases.append((f"{spp} spp, {'Philox' if mode else 'PCG'}", poses, frames, accum))
    frame_rmse = [denoise_check.rmse(c[2][-1], converged) for c in cases]
    accum_rmse = [denoise_check.rmse(c[3], converged) for c in cases]
    rows = []
    for mh, dt, nt in itertools.product((2, 4, 8, 16, 32, 64), (0.01, 0.05, 0.2), (0.1, 0.5, 1.5)):
        ratios = []
        for (label, poses, frames, _), fr in zip(cases, frame_rmse):
            chk = temporal_check.Checker()
            for p, f, g in zip(poses, frames, guides):
                T, _ = chk.step(f, *g, p, maxHistory=mh, depthTolerance=dt, normalTolerance=nt)
            ratios.append(denoise_check.rmse(T, converged) / fr)
        rows.append((float(np.mean(ratios)), mh, dt, nt, ratios))
    rows.sort(key=lambda r: r[0])
    lines = [f"Temporal reprojection defaults: sweep on mesh_test_scene {q.QW}x{q.QH}, a path of {q.POSES} poses (step {q.PATH_STEP}, yaw {q.PATH_YAW} per pose),",
             "one frame per pose, 4 feature frames per pose, against a converged oracle image of the last pose (1024 samples per pixel, Philox mode).",
             "CPU: oracle + tests/aov_oracle.c + tests/temporal_oracle.c.  ratio = RMSE(T) / RMSE(single frame) at the last pose; score = mean of the",
             "four ratios; sorted by score.  A path of 8 poses cannot tell history caps of 8 and above apart, and the tolerances from 0.05 / 0.5",
             "upwards differ by less than the cases do among themselves (0.3 % of the score), while wider tolerances admit history across",
             "surfaces, which a static scene cannot punish: the starting values maxHistory 32, depthTolerance 0.05, normalTolerance 0.5 are",
             "confirmed as the defaults (their row is marked).",
             "",
             "single frame RMSE:       " + ", ".join(f"{c[0]}: {r:.4f}" for c, r in zip(cases, frame_rmse)),
             "plain accumulation RMSE: " + ", ".join(f"{c[0]}: {r:.4f}" for c, r in zip(cases, accum_rmse)),
             "",
             "score   maxHistory depthTolerance normalTolerance | " + " | ".join(c[0] for c in cases)]
    for score, mh, dt, nt, ratios in rows:
        mark = "   <- defaults" if (mh, dt, nt) == (32, 0.05, 0.5) else ""
        lines.append(f"{score:.4f}  {mh:10d} {dt:14.2f} {nt:15.2f} | " + " | ".join(f"{r:.4f}" for r in ratios) + mark)
    with open(os.path.join(ROOT, "profiles", "temporal_defaults.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:24]))


if __name__ == "__main__":
    main()
