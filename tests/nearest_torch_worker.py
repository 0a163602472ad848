"""Child process of tests/test_gpu_nearest.py: rt_closest_points_device with the options "closest_k" / "closest_all" on torch tensors
gives the checker's bits as an (n, K, 16) tensor, on torch's default stream and on a stream of its own, with and without the counting
kernel; nearest.py's helpers take tensors; at the defaults the tensor is (n, 16) again.  torch is imported before the library is
loaded (torch brings its own HIP runtime; the library then uses it), so it runs in a fresh process."""
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
    import nearest_check as nc
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    rng = np.random.default_rng(13)
    lo, hi = tr["posA"].min(0), tr["posA"].max(0)
    n = 150
    pts = cc.points_of(rtx, lo - (hi - lo) * 0.25 + rng.random((n, 3)) * 1.5 * (hi - lo))
    pts["tMax"][::9] = 0.0
    pts["tMax"][1::9] = 0.75
    pts["origin"][5] *= np.float32(1e4)                          # the device entry measures the origin bound itself
    pts = np.concatenate([nc.vertex_tie_points(rtx, s, tr, mi, 40), pts])
    n = len(pts)
    as_records = lambda t, k: t.cpu().numpy().view(rtx.CLOSEST).reshape(-1, k)     # noqa: E731
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        t.set_option("closest_slice", 70)                        # three launches per call
        dev = torch.from_numpy(pts.view(np.float32).reshape(-1, 8).copy()).cuda()
        default = t.closest_points(dev)
        assert tuple(default.shape) == (n, 16)
        cc.assert_same_records(rtx, as_records(default, 1)[:, 0], cc.oracle_closest(rtx, s, tr, mi, pts), "defaults")
        for k, count_all in nc.FORMS:
            want = nc.oracle_nearest(rtx, s, tr, mi, pts, k, count_all)
            t.set_option("closest_k", k)
            t.set_option("closest_all", count_all)
            got = t.closest_points_device(dev)
            assert (tuple(got.shape) == ((n, k, 16) if k > 1 else (n, 16))) and got.dtype == torch.float32 and got.is_cuda
            nc.assert_same_records(rtx, as_records(got, k), want, f"default stream, K {k} all {count_all}")
            t.set_option("closest_count", 1)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                d2 = dev * 1.0                                   # written on the side stream, read by the query on it
                got2 = t.closest_points(d2)
                counted = t.closest_info()                       # (waits for the stream once, for the counts)
                got2 = got2.cpu()
            nc.assert_same_records(rtx, as_records(got2, k), want, f"side stream, counting kernel, K {k} all {count_all}")
            assert counted["lastPrimTests"] >= int((pts["tMax"] > 0).sum()) * len(s) and counted["lastNodeSteps"] > 0, counted
            t.set_option("closest_count", 0)
            t.set_option("closest_k", 1)
            t.set_option("closest_all", 0)
            # the helpers on a tensor
            got3 = rtx.nearest.nearest_k(t, dev, k, count_all=bool(count_all))
            assert tuple(got3.shape) == (n, k, 16)
            nc.assert_same_records(rtx, as_records(got3, k), want, f"nearest_k(tensor), K {k} all {count_all}")
        R = np.float32(0.75)
        counts = rtx.nearest.overlap_count(t, dev, float(R))
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (n,)
        q = pts.copy()
        q["tMax"] = R
        want = nc.oracle_nearest(rtx, s, tr, mi, q, 1, 1)["_reserved"][:, 0, 0]
        assert np.array_equal(counts.cpu().numpy(), want) and want.max() > 1
        assert tuple(t.closest_points(dev).shape) == (n, 16)     # the helpers put the defaults back
    print("nearest device entry ok")


if __name__ == "__main__":
    main()
