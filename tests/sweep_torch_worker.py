"""Child process of tests/test_gpu_sweep.py and test_gpu_sweep_all.py: sweep_torch_worker.py <cast|cast_all>.
cast: with option "sweep" = 1 rt_trace_rays_device and rt_occluded_device on torch tensors give the host entries' bits, and
sweep.sphere_cast / sphere_check take a tensor and a tensor of radii.  cast_all: the same of rt_trace_hits_device with option
"hits_sweep" = 1 and sweep.sphere_cast_all.  Both on torch's default stream and on a stream of its own.  torch is imported before the
library is loaded (torch brings its own HIP runtime; the library then uses it), so it runs in a fresh process."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


# ---- per word: what the checker says of the batch, and the checks of the helpers on tensors; `side` runs a call on a stream of its own
def cast(rtx, t, s, tr, mi, rays, radii, one, dev, side):
    import sweep_check as sc
    want, occ = sc.oracle_cast(rtx, s, tr, mi, rays)
    assert 100 < (want["kind"] != 0).sum() < len(want) - 100
    sc.assert_same_records(rtx, rtx.sweep.sphere_cast(t, rays, radii), want, "host entry")
    got = rtx.sweep.sphere_cast(t, dev, torch.from_numpy(radii).cuda())
    assert tuple(got.shape) == (len(rays), 16) and got.dtype == torch.float32 and got.is_cuda
    sc.assert_same_records(rtx, got.cpu().numpy().view(rtx.HIT).reshape(-1), want, "default stream")
    chk = rtx.sweep.sphere_check(t, dev, radii)              # (host radii for a tensor of rays)
    assert chk.dtype == torch.uint8 and np.array_equal(chk.cpu().numpy(), occ)
    got2 = side(lambda d2: rtx.sweep.sphere_cast(t, d2, float(radii[0])))
    sc.assert_same_records(rtx, got2.numpy().view(rtx.HIT).reshape(-1), sc.oracle_cast(rtx, s, tr, mi, one)[0], "side stream, one radius")
    return lambda r: t.trace_rays(r), rtx.HIT, (len(rays),)


def cast_all(rtx, t, s, tr, mi, rays, radii, one, dev, side):
    import sweep_all_check as sac
    want = sac.oracle_cast_all(rtx, s, tr, mi, rays, 8, True)
    assert (want[:, 0]["hitCount"] > 8).sum() > 16 and (want[:, 0]["hitCount"] == 0).sum() > 100

    def records(tensor, K):
        assert tuple(tensor.shape) == (len(rays), K, 16) and tensor.dtype == torch.float32 and tensor.is_cuda
        return tensor.cpu().numpy().view(rtx.MULTIHIT).reshape(len(rays), K)
    sac.assert_same_records(rtx, rtx.sweep.sphere_cast_all(t, rays, radii, 8, True), want, "host entry")
    got = rtx.sweep.sphere_cast_all(t, dev, torch.from_numpy(radii).cuda(), 8, True)
    sac.assert_same_records(rtx, records(got, 8), want, "default stream")
    got3 = rtx.sweep.sphere_cast_all(t, dev, radii, 3)       # (host radii for a tensor of rays)
    sac.assert_same_records(rtx, records(got3, 3), sac.oracle_cast_all(rtx, s, tr, mi, rays, 3, False), "K = 3")
    got2 = side(lambda d2: rtx.sweep.sphere_cast_all(t, d2, float(radii[0]), 4, True))
    sac.assert_same_records(rtx, got2.numpy().view(rtx.MULTIHIT).reshape(len(rays), 4), sac.oracle_cast_all(rtx, s, tr, mi, one, 4, True),
                            "side stream, one radius")
    return lambda r: t.trace_hits(r, 4), rtx.MULTIHIT, (len(rays), 4)


WORK = {"cast": (cast, "sweep device entry ok"), "cast_all": (cast_all, "sweep-all device entry ok")}


def main(word):
    import rtx_pkg
    rtx = rtx_pkg.load()
    import sweep_check as sc
    checks, ok = WORK[word]
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    rays, _ = sc.batch_of(rtx, s, tr, mi, seed=13)
    radii = sc.radii_of(rays).copy()
    one = rays.copy()
    one["_reserved"] = radii[:1].view(np.int32)[0]
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        keep = dev.clone()

        def side(call):
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                return call(dev * 1.0).cpu()                     # written on the side stream, read by the query on it
        plain_call, record, shape = checks(rtx, t, s, tr, mi, rays, radii, one, dev, side)
        assert torch.equal(dev.view(torch.int32), keep.view(torch.int32))      # the radii went into a copy (words: the batch holds NaNs)
        # the option is back at 0: the same tensor is a batch of plain rays again
        plain = plain_call(dev).cpu().numpy().view(record).reshape(shape)
        assert plain.tobytes() == plain_call(rays).tobytes() and (plain["_reserved"] == 0).all()
    print(ok)


if __name__ == "__main__":
    main(sys.argv[1])
