"""Child process of tests/test_gpu_sweep.py: with option "sweep" = 1 rt_trace_rays_device and rt_occluded_device on torch tensors give
the host entries' bits, on torch's default stream and on a stream of its own, and sweep.sphere_cast / sphere_check take a tensor and a
tensor of radii.  torch is imported before the library is loaded (torch brings its own HIP runtime; the library then uses it), so it
runs in a fresh process."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import rtx_pkg
    rtx = rtx_pkg.load()
    import sweep_check as sc
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    rays, _ = sc.batch_of(rtx, s, tr, mi, seed=13)
    radii = sc.radii_of(rays).copy()
    want, occ = sc.oracle_cast(rtx, s, tr, mi, rays)
    assert 100 < (want["kind"] != 0).sum() < len(want) - 100
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        sc.assert_same_records(rtx, rtx.sweep.sphere_cast(t, rays, radii), want, "host entry")
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        keep = dev.clone()
        got = rtx.sweep.sphere_cast(t, dev, torch.from_numpy(radii).cuda())
        assert tuple(got.shape) == (len(rays), 16) and got.dtype == torch.float32 and got.is_cuda
        sc.assert_same_records(rtx, got.cpu().numpy().view(rtx.HIT).reshape(-1), want, "default stream")
        chk = rtx.sweep.sphere_check(t, dev, radii)              # (host radii for a tensor of rays)
        assert chk.dtype == torch.uint8 and np.array_equal(chk.cpu().numpy(), occ)
        assert torch.equal(dev.view(torch.int32), keep.view(torch.int32))      # the radii went into a copy (words: the batch holds NaNs)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d2 = dev * 1.0                                       # written on the side stream, read by the query on it
            got2 = rtx.sweep.sphere_cast(t, d2, float(radii[0])).cpu()
        one = rays.copy()
        one["_reserved"] = radii[:1].view(np.int32)[0]
        sc.assert_same_records(rtx, got2.numpy().view(rtx.HIT).reshape(-1), sc.oracle_cast(rtx, s, tr, mi, one)[0], "side stream, one radius")
        # the option is back at 0: the same tensor is a batch of plain rays again
        plain = t.trace_rays(dev).cpu().numpy().view(rtx.HIT).reshape(-1)
        assert plain.tobytes() == t.trace_rays(rays).tobytes() and (plain["_reserved"] == 0).all()
    print("sweep device entry ok")


if __name__ == "__main__":
    main()
