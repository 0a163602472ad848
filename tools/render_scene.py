#!/usr/bin/env python3
"""Render one of the reference's scenes (a Unity .unity file, or a tests/golden/scenes/*.npz conversion of one) on the
MI355X tracer and write what the reference shows on screen: the accumulated resultTexture after N frames
(RayTracingManager.OnRenderImage, Assets/Scripts/RayTracingManager.cs:49-93) as sRGB PNG (the back-buffer blit :84) and,
optionally, the linear RGBA32F image as OpenEXR / PFM.

    python tools/render_scene.py Assets/Scenes/Chess.unity --frames 16 --png chess.png --exr chess.exr
    python tools/render_scene.py tests/golden/scenes/Knight.npz --width 960 --height 540 --rays 16 --frames 4 --png k.png
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", help=".unity scene of the reference project, or an .npz written by unity_scene.save_scene_npz")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=16, help="frames to accumulate (spp = frames x rays per pixel)")
    ap.add_argument("--rays", type=int, default=0, help="override numRaysPerPixel of the scene's RayTracingManager")
    ap.add_argument("--bounces", type=int, default=0, help="override maxBounceCount")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--png"); ap.add_argument("--exr"); ap.add_argument("--pfm")
    ap.add_argument("--aov", metavar="PREFIX", help="also accumulate the feature buffers over the same frames (rt_render_aov) and write PREFIX.albedo "
                    "(albedo, alpha = coverage), PREFIX.normal (mean shading normal, alpha = coverage) and PREFIX.depth (mean depth in every "
                    "channel, alpha = coverage), as .exr, or as .pfm when --pfm is given and --exr is not")
    ap.add_argument("--denoise", nargs="?", const="atrous", choices=("atrous", "variance"), help="after the frames (and the feature frames: accumulated "
                    "over the same frames even without --aov) run rt_denoise (--denoise or --denoise atrous) or the variance-guided "
                    "rt_denoise_variance (--denoise variance) with the library's defaults and write the denoised image beside the noisy one: "
                    "NAME.denoised.EXT for every --png / --exr / --pfm given")
    ap.add_argument("--temporal", type=int, default=0, metavar="POSES", help="after the image: a camera path of POSES poses, each --temporal-step "
                    "world units further along the camera's right axis; at every pose a fresh accumulation of --temporal-frames frames, fresh "
                    "feature frames, rt_temporal and rt_denoise_temporal with the library's defaults.  Writes, for the last pose, "
                    "NAME.temporal.EXT and NAME.temporal.denoised.EXT for every --png / --exr / --pfm given")
    ap.add_argument("--temporal-step", type=float, default=0.05)
    ap.add_argument("--temporal-frames", type=int, default=1, help="frames per pose of the camera path")
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    from rtx_amd import unity_scene
    tracer = rtx.Tracer(args.device)                  # raises if the HIP library or a GPU is missing: there is no CPU path
    if args.scene.endswith(".npz"):
        mgr = unity_scene.load_scene_npz(args.scene, args.width, args.height, backend=tracer)
    else:
        mgr = unity_scene.load_unity_scene(args.scene, args.width, args.height, backend=tracer)
    if args.rays:
        mgr.numRaysPerPixel = args.rays
    if args.bounces:
        mgr.maxBounceCount = args.bounces
    t0 = time.time()
    image = mgr.OnRenderImage(frames=args.frames)
    dt = time.time() - t0
    st = tracer.stats()
    print(f"{os.path.basename(args.scene)}: {args.width}x{args.height}, {mgr.numRaysPerPixel} rays/pixel x {args.frames} frames, "
          f"{mgr.maxBounceCount} bounces; {mgr.numTriangles} triangles in {mgr.numMeshChunks} chunks; "
          f"{st['rays']:,} rays in {st['totalKernelMs']:.1f} ms of kernels ({dt:.2f} s with scene upload and BVH build)")
    if args.png:
        rtx.imageio.write_png(args.png, tracer.read_display())
    if args.exr:
        rtx.imageio.write_exr(args.exr, image)
    if args.pfm:
        rtx.imageio.write_pfm(args.pfm, image)
    if args.aov:
        import numpy as np
        albedo, normal_depth = mgr.RenderFeatures(frames=args.frames, firstFrame=0)
        info = tracer.aov_info()
        coverage = albedo[..., 3:4]
        planes = {"albedo": albedo, "normal": np.concatenate([normal_depth[..., :3], coverage], -1),
                  "depth": np.concatenate([np.repeat(normal_depth[..., 3:4], 3, -1), coverage], -1)}
        ext, write = (".pfm", rtx.imageio.write_pfm) if (args.pfm and not args.exr) else (".exr", rtx.imageio.write_exr)
        for name, plane in planes.items():
            write(f"{args.aov}.{name}{ext}", np.ascontiguousarray(plane, np.float32))
        print(f"feature buffers: {info['framesAccumulated']} frames in {info['totalKernelMs']:.1f} ms of kernels "
              f"({info['lastSampleLanes']} lanes per pixel) -> {args.aov}.{{albedo,normal,depth}}{ext}")
    if args.denoise:
        if not args.aov:
            mgr.RenderFeatures(frames=args.frames, firstFrame=0)
        if args.denoise == "variance":
            denoised, _ = mgr.DenoiseVariance()
            info = tracer.vdenoise_info()
        else:
            denoised = mgr.Denoise()
            info = tracer.denoise_info()

        def beside(path):
            stem, ext = os.path.splitext(path)
            return stem + ".denoised" + ext
        written = []
        if args.png:
            rtx.imageio.write_png(beside(args.png), tracer.read_denoised_display()); written.append(beside(args.png))
        if args.exr:
            rtx.imageio.write_exr(beside(args.exr), denoised); written.append(beside(args.exr))
        if args.pfm:
            rtx.imageio.write_pfm(beside(args.pfm), denoised); written.append(beside(args.pfm))
        print(f"denoised: {info['iterations']} passes in {info['lastKernelMs']:.3f} ms of kernels -> {', '.join(written) or 'nothing written (give --png, --exr or --pfm)'}")
    if args.temporal > 0:
        import numpy as np
        cam = mgr.camera.transform
        start = np.array(cam.position, np.float32)
        right = cam.localToWorldMatrix[:3, 0]
        right = right / np.linalg.norm(right)
        tracer.reset_temporal()
        for pose in range(args.temporal):
            cam.position = (start + right * np.float32(args.temporal_step * pose)).astype(np.float32)
            mgr.Start()                                     # a fresh accumulation at the new pose
            mgr.OnRenderImage(frames=args.temporal_frames)
            tracer.reset_aov()
            mgr.RenderFeatures(frames=args.temporal_frames, firstFrame=0)
            temporal = mgr.Temporal()
        tracer.denoise_temporal()
        denoised, info, history = tracer.read_denoised(), tracer.temporal_info(), tracer.read_temporal_history()
        cam.position = start
        written = []
        for path, kind in ((args.png, "png"), (args.exr, "exr"), (args.pfm, "pfm")):
            if not path:
                continue
            stem, ext = os.path.splitext(path)
            if kind == "png":
                rtx.imageio.write_png(stem + ".temporal" + ext, tracer.read_temporal_display())
                rtx.imageio.write_png(stem + ".temporal.denoised" + ext, tracer.read_denoised_display())
            else:
                write = rtx.imageio.write_exr if kind == "exr" else rtx.imageio.write_pfm
                write(stem + ".temporal" + ext, temporal)
                write(stem + ".temporal.denoised" + ext, denoised)
            written += [stem + ".temporal" + ext, stem + ".temporal.denoised" + ext]
        print(f"temporal: {info['calls']} poses, {args.temporal_frames} frames each, {info['totalKernelMs']:.3f} ms of kernels for the step; mean history "
              f"length {float(history.mean()):.2f} -> {', '.join(written) or 'nothing written (give --png, --exr or --pfm)'}")
    tracer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
