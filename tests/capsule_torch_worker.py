"""Child process of tests/test_gpu_capsule.py: rt_closest_points_device with the option "closest_capsule" on torch tensors gives the
checker's bits as an (n, K, 16) tensor, on torch's default stream and on a stream of its own, with and without the counting kernel;
the device path's origin bound sees both endpoints; capsule.py's helpers take tensors; at the defaults the tensor is the closest-point
call's again.  torch is imported before the library is loaded (torch brings its own HIP runtime; the library then uses it), so it runs
in a fresh process."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import rtx_pkg
    rtx = rtx_pkg.load()
    import capsule_check as kc
    import closest_check as cc
    from test_gpu_closest import batch_of
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    segs = kc.batch_of(rtx, s, tr, mi, batch_of(rtx, s, tr, mi)[::3], per_kind=12)
    n = len(segs)
    as_records = lambda t, k: t.cpu().numpy().view(rtx.CLOSEST).reshape(-1, k)     # noqa: E731
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        t.set_option("closest_slice", 70)                        # several launches per call
        dev = torch.from_numpy(segs.view(np.float32).reshape(-1, 8).copy()).cuda()
        default = t.closest_points(dev)
        assert tuple(default.shape) == (n, 16)
        cc.assert_same_records(rtx, as_records(default, 1)[:, 0], cc.oracle_closest(rtx, s, tr, mi, segs), "defaults before")
        for k, count_all in kc.FORMS:
            want = kc.oracle_capsule(rtx, s, tr, mi, segs, k, count_all)
            t.set_option("closest_capsule", 1)
            t.set_option("closest_k", k)
            t.set_option("closest_all", count_all)
            got = t.closest_points_device(dev)
            assert (tuple(got.shape) == ((n, k, 16) if k > 1 else (n, 16))) and got.dtype == torch.float32 and got.is_cuda
            kc.assert_same_records(rtx, as_records(got, k), want, f"default stream, K {k} all {count_all}")
            t.set_option("closest_count", 1)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                d2 = dev * 1.0                                   # written on the side stream, read by the query on it
                got2 = t.closest_points(d2)
                counted = t.closest_info()                       # (waits for the stream once, for the counts)
                got2 = got2.cpu()
            kc.assert_same_records(rtx, as_records(got2, k), want, f"side stream, counting kernel, K {k} all {count_all}")
            assert counted["lastPrimTests"] >= int(kc.counts(want)[:, 0].sum()) and counted["lastNodeSteps"] > 0, counted
            t.set_option("closest_count", 0)
            t.set_option("closest_capsule", 0)
            t.set_option("closest_k", 1)
            t.set_option("closest_all", 0)
        # the helpers on tensors (finite inputs: the helper forms d = p1 - p0 again)
        ok = np.isfinite(segs["origin"]).all(1) & np.isfinite(segs["direction"]).all(1) & (np.abs(segs["origin"]) < 1e30).all(1)
        p0 = dev[torch.from_numpy(ok).cuda(), 0:3].contiguous()
        p1 = p0 + dev[torch.from_numpy(ok).cuda(), 4:7]
        again_segs = kc.segments_of(rtx, p0.cpu().numpy(), p1.cpu().numpy(), 1.5)
        got3 = rtx.capsule.overlap_capsule(t, p0, p1, 1.5, 4, count_all=True)
        assert tuple(got3.shape) == (int(ok.sum()), 4, 16)
        kc.assert_same_records(rtx, as_records(got3, 4), kc.oracle_capsule(rtx, s, tr, mi, again_segs, 4, 1), "overlap_capsule(tensor)")
        any_ = rtx.capsule.check_capsule(t, p0, p1, 1.5)
        want = kc.counts(kc.oracle_capsule(rtx, s, tr, mi, again_segs, 1, 0))[:, 0] != 0
        assert any_.dtype == torch.uint8 and np.array_equal(any_.cpu().numpy(), want.astype(np.uint8)) and 0 < want.sum() < len(want)
        rec, par = rtx.capsule.closest_to_segment(t, p0, p1)
        again_segs["tMax"] = np.inf
        want = kc.oracle_capsule(rtx, s, tr, mi, again_segs, 1, 0)
        kc.assert_same_records(rtx, as_records(rec, 1), want, "closest_to_segment(tensor)")
        assert np.array_equal(par.cpu().numpy().view(np.uint32), kc.params(want)[:, 0].view(np.uint32))
        # the device path's origin bound: P0 near the scene, P1 1e8 away (beyond everything the batch above reached) widens the padding once
        far = kc.segments_of(rtx, again_segs["origin"][:130], d=np.repeat(np.float32([[1e8, 0, -7e7]]), 130, 0), radius=2.0)
        before = t.stats()["bvhRepads"]
        fdev = torch.from_numpy(far.view(np.float32).reshape(-1, 8).copy()).cuda()
        t.closest_points(fdev)                                   # as points: nothing moves
        assert t.stats()["bvhRepads"] == before
        got4 = rtx.capsule.overlap_capsule(t, fdev[:, 0:3].contiguous(), fdev[:, 0:3] + fdev[:, 4:7], 2.0, 8)
        far = kc.segments_of(rtx, far["origin"], far["origin"] + far["direction"], 2.0)
        kc.assert_same_records(rtx, as_records(got4, 8), kc.oracle_capsule(rtx, s, tr, mi, far, 8, 0), "P1 far away, device entry")
        assert t.stats()["bvhRepads"] == before + 1
        again = t.closest_points(dev)                            # the helpers put the defaults back
        assert tuple(again.shape) == (n, 16) and torch.equal(again.view(torch.int32), default.view(torch.int32))
    print("capsule device entry ok")


if __name__ == "__main__":
    main()
