"""Child process of tests/test_gpu_overlap.py: rt_closest_points_device with the option "closest_box" on torch tensors gives the
checker's bits as an (n, K, 16) tensor, on torch's default stream and on a stream of its own, with and without the counting kernel;
overlap.py's helpers take tensors; at the defaults the tensor is the closest-point call's again.  torch is imported before the library
is loaded (torch brings its own HIP runtime; the library then uses it), so it runs in a fresh process."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import rtx_pkg
    rtx = rtx_pkg.load()
    import closest_check as cc
    import overlap_check as oc
    from test_gpu_closest import batch_of
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    boxes = oc.batch_of(rtx, s, tr, mi, batch_of(rtx, s, tr, mi)[::3], per_kind=12)
    n = len(boxes)
    as_records = lambda t, k: t.cpu().numpy().view(rtx.CLOSEST).reshape(-1, k)     # noqa: E731
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        t.set_option("closest_slice", 70)                        # several launches per call
        dev = torch.from_numpy(boxes.view(np.float32).reshape(-1, 8).copy()).cuda()
        default = t.closest_points(dev)
        assert tuple(default.shape) == (n, 16)
        cc.assert_same_records(rtx, as_records(default, 1)[:, 0], cc.oracle_closest(rtx, s, tr, mi, boxes), "defaults before")
        for k, count_all in oc.FORMS:
            want = oc.oracle_overlap(rtx, s, tr, mi, boxes, k, count_all)
            t.set_option("closest_box", 1)
            t.set_option("closest_k", k)
            t.set_option("closest_all", count_all)
            got = t.closest_points_device(dev)
            assert (tuple(got.shape) == ((n, k, 16) if k > 1 else (n, 16))) and got.dtype == torch.float32 and got.is_cuda
            oc.assert_same_records(rtx, as_records(got, k), want, f"default stream, K {k} all {count_all}")
            t.set_option("closest_count", 1)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                d2 = dev * 1.0                                   # written on the side stream, read by the query on it
                got2 = t.closest_points(d2)
                counted = t.closest_info()                       # (waits for the stream once, for the counts)
                got2 = got2.cpu()
            oc.assert_same_records(rtx, as_records(got2, k), want, f"side stream, counting kernel, K {k} all {count_all}")
            assert counted["lastPrimTests"] >= int(oc.counts(want)[:, 0].sum()) and counted["lastNodeSteps"] > 0, counted
            t.set_option("closest_count", 0)
            t.set_option("closest_box", 0)
            t.set_option("closest_k", 1)
            t.set_option("closest_all", 0)
            # the helpers on tensors
            got3 = rtx.overlap.overlap_box(t, dev[:, 0:3].contiguous(), dev[:, 4:7].contiguous(), k, count_all=bool(count_all))
            assert tuple(got3.shape) == (n, k, 16)
            gate = boxes.copy()
            gate["tMax"] = 1.0                                   # (the helper's gate is always open)
            oc.assert_same_records(rtx, as_records(got3, k), oc.oracle_overlap(rtx, s, tr, mi, gate, k, count_all), f"overlap_box(tensor), K {k} all {count_all}")
        any_ = rtx.overlap.check_box(t, dev[:, 0:3].contiguous(), dev[:, 4:7].contiguous())
        assert any_.dtype == torch.uint8 and tuple(any_.shape) == (n,)
        want = (oc.counts(oc.oracle_overlap(rtx, s, tr, mi, gate, 1, 0))[:, 0] != 0)
        assert np.array_equal(any_.cpu().numpy(), want.astype(np.uint8)) and 0 < want.sum() < n
        again = t.closest_points(dev)                            # the helpers put the defaults back
        assert tuple(again.shape) == (n, 16) and torch.equal(again.view(torch.int32), default.view(torch.int32))
    print("overlap device entry ok")


if __name__ == "__main__":
    main()
