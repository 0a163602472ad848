"""Child process of tests/test_gpu_closest.py: rt_closest_points_device on torch tensors gives the host entry's bits, on torch's default
stream and on a stream of its own, with and without the counting kernel; a misaligned pointer and host memory are refused;
rt_closest_info counts the calls.  torch is imported before the library is loaded (torch brings its own HIP runtime; the library then
uses it), so it runs in a fresh process."""
import ctypes
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
    lib = rtx.load_library()
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    rng = np.random.default_rng(13)
    lo, hi = tr["posA"].min(0), tr["posA"].max(0)
    n = 150
    pts = cc.points_of(rtx, lo - (hi - lo) * 0.25 + rng.random((n, 3)) * 1.5 * (hi - lo))
    pts["tMax"][::9] = 0.0
    pts["tMax"][1::9] = 0.75
    pts["origin"][5] *= np.float32(1e4)                          # the device entry measures the origin bound itself
    want = cc.oracle_closest(rtx, s, tr, mi, pts)
    assert (want["kind"][::9] == 0).all() and len(np.unique(want["primitive"])) > 5 and 0 < (want["kind"][1::9] == 0).sum() < len(want[1::9])
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        t.set_option("closest_slice", 70)                        # three launches per call
        host = t.closest_points(pts)
        cc.assert_same_records(rtx, host, want, "host entry")
        info = t.closest_info()
        assert info["calls"] == 1 and info["lastKernelMs"] > 0 and info["totalKernelMs"] >= info["lastKernelMs"], info
        dev = torch.from_numpy(pts.view(np.float32).reshape(-1, 8).copy()).cuda()
        got = t.closest_points_device(dev)
        assert tuple(got.shape) == (n, 16) and got.dtype == torch.float32 and got.is_cuda
        cc.assert_same_records(rtx, got.cpu().numpy().view(rtx.CLOSEST).reshape(-1), want, "default stream")
        after = t.closest_info()
        assert after["calls"] == 2 and after["lastKernelMs"] == info["lastKernelMs"] and after["totalKernelMs"] == info["totalKernelMs"], after
        t.set_option("closest_count", 1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d2 = dev * 1.0                                       # written on the side stream, read by the query on it
            got2 = t.closest_points(d2)
            counted = t.closest_info()                           # (waits for the stream once, for the counts)
            got2 = got2.cpu()
        cc.assert_same_records(rtx, got2.numpy().view(rtx.CLOSEST).reshape(-1), want, "side stream, counting kernel")
        searched = int((pts["tMax"] > 0).sum())
        assert counted["calls"] == 3 and counted["lastPrimTests"] >= searched * len(s) and counted["lastNodeSteps"] >= searched, counted
        t.set_option("closest_count", 0)
        # the manager's method reaches the same entry with a tensor
        mgr.backend = t
        got3 = mgr.ClosestPoints(dev)
        cc.assert_same_records(rtx, got3.cpu().numpy().view(rtx.CLOSEST).reshape(-1), want, "ClosestPoints(tensor)")
        assert t.closest_info()["lastPrimTests"] == 0
        # refusals: a misaligned device pointer (points, then out), host memory on either side
        vp = ctypes.c_void_p
        out = torch.full((n, 16), 7.0, dtype=torch.float32, device=dev.device)
        torch.cuda.synchronize()
        table = [
            ("misaligned points", vp(dev.data_ptr() + 4), vp(out.data_ptr()), b"aligned"),
            ("misaligned out", vp(dev.data_ptr()), vp(out.data_ptr() + 8), b"aligned"),
            ("host out", vp(dev.data_ptr()), np.zeros((8, 16), np.float32).ctypes.data_as(vp), b"device"),
            ("host points", pts.ctypes.data_as(vp), vp(out.data_ptr()), b"device"),
        ]
        for label, a, b, word in table:
            assert lib.rt_closest_points_device(t._ctx, a, 8, b) == -2, label
            assert word in lib.rt_last_error(t._ctx), (label, lib.rt_last_error(t._ctx))
        assert t.closest_info()["calls"] == 4 and bool((out == 7.0).all())
    print("closest device entry ok")


if __name__ == "__main__":
    main()
