"""Child process of tests/test_gpu_sweep_all.py: with option "hits_sweep" = 1 rt_trace_hits_device on torch tensors gives the host entry's
bits, on torch's default stream and on a stream of its own, and sweep.sphere_cast_all takes a tensor and a tensor of radii.  torch is
imported before the library is loaded (torch brings its own HIP runtime; the library then uses it), so it runs in a fresh process."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import rtx_pkg
    rtx = rtx_pkg.load()
    import sweep_all_check as sac
    import sweep_check as sc
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    rays, _ = sc.batch_of(rtx, s, tr, mi, seed=13)
    radii = sc.radii_of(rays).copy()
    want = sac.oracle_cast_all(rtx, s, tr, mi, rays, 8, True)
    assert (want[:, 0]["hitCount"] > 8).sum() > 16 and (want[:, 0]["hitCount"] == 0).sum() > 100

    def records(tensor, K):
        assert tuple(tensor.shape) == (len(rays), K, 16) and tensor.dtype == torch.float32 and tensor.is_cuda
        return tensor.cpu().numpy().view(rtx.MULTIHIT).reshape(len(rays), K)
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        sac.assert_same_records(rtx, rtx.sweep.sphere_cast_all(t, rays, radii, 8, True), want, "host entry")
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        keep = dev.clone()
        got = rtx.sweep.sphere_cast_all(t, dev, torch.from_numpy(radii).cuda(), 8, True)
        sac.assert_same_records(rtx, records(got, 8), want, "default stream")
        got3 = rtx.sweep.sphere_cast_all(t, dev, radii, 3)       # (host radii for a tensor of rays)
        sac.assert_same_records(rtx, records(got3, 3), sac.oracle_cast_all(rtx, s, tr, mi, rays, 3, False), "K = 3")
        assert torch.equal(dev.view(torch.int32), keep.view(torch.int32))      # the radii went into a copy (words: the batch holds NaNs)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d2 = dev * 1.0                                       # written on the side stream, read by the query on it
            got2 = rtx.sweep.sphere_cast_all(t, d2, float(radii[0]), 4, True).cpu()
        one = rays.copy()
        one["_reserved"] = radii[:1].view(np.int32)[0]
        sac.assert_same_records(rtx, got2.numpy().view(rtx.MULTIHIT).reshape(len(rays), 4), sac.oracle_cast_all(rtx, s, tr, mi, one, 4, True),
                                "side stream, one radius")
        # the option is back at 0: the same tensor is a batch of plain rays again
        plain = t.trace_hits(dev, 4).cpu().numpy().view(rtx.MULTIHIT).reshape(len(rays), 4)
        assert plain.tobytes() == t.trace_hits(rays, 4).tobytes() and (plain["_reserved"] == 0).all()
    print("sweep-all device entry ok")


if __name__ == "__main__":
    main()
