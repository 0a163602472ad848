"""Child process of tests/test_gpu_hits.py: rt_trace_hits_device on torch tensors gives the host entry's bits, on torch's default stream
and on a stream of its own; a misaligned pointer and host memory are refused; rt_hits_info counts the calls.  torch is imported before
the library is loaded (torch brings its own HIP runtime; the library then uses it), so it runs in a fresh process."""
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
    import hits_check as hc
    lib = rtx.load_library()
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    rays = hc.batch_of(rtx, s, tr, mi, seed=13)[::7].copy()
    rays["origin"][5] *= np.float32(1e4)                         # the device entry measures the origin bound itself
    n = len(rays)

    def records(tensor, K):
        return tensor.cpu().numpy().view(rtx.MULTIHIT).reshape(n, K)
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        t.set_option("hits_slice", 150)                          # three launches per call
        want = hc.oracle_hits(rtx, s, tr, mi, rays, 3, hc.BOTH, True)
        assert (want["kind"] != 0).sum() > n // 4 and (want["side"] == -1).sum() > 10
        host = t.trace_hits(rays, 3, True, True)
        hc.assert_same_records(rtx, host, want, "host entry")
        info = t.hits_info()
        assert info["calls"] == 1 and info["lastKernelMs"] > 0 and info["totalKernelMs"] >= info["lastKernelMs"], info
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        got = t.trace_hits_device(dev, 3, True, True)
        assert tuple(got.shape) == (n, 3, 16) and got.dtype == torch.float32 and got.is_cuda
        hc.assert_same_records(rtx, records(got, 3), want, "default stream")
        after = t.hits_info()
        assert after["calls"] == 2 and after["lastKernelMs"] == info["lastKernelMs"] and after["totalKernelMs"] == info["totalKernelMs"], after
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d2 = dev * 1.0                                       # written on the side stream, read by the query on it
            got2 = t.trace_hits(d2, 8).cpu()
        hc.assert_same_records(rtx, got2.numpy().view(rtx.MULTIHIT).reshape(n, 8), hc.oracle_hits(rtx, s, tr, mi, rays, 8), "side stream, K = 8")
        assert (t.hits_info()["lastMaxHits"], t.hits_info()["lastMode"], t.hits_info()["lastCountAll"]) == (8, 0, 0)
        # refusals: a misaligned device pointer (rays, then out), host memory on either side
        vp = ctypes.c_void_p
        out = torch.full((n, 4, 16), 7.0, dtype=torch.float32, device=dev.device)
        torch.cuda.synchronize()
        table = [
            ("misaligned rays", vp(dev.data_ptr() + 4), vp(out.data_ptr()), b"aligned"),
            ("misaligned out", vp(dev.data_ptr()), vp(out.data_ptr() + 8), b"aligned"),
            ("host out", vp(dev.data_ptr()), np.zeros((8, 4, 16), np.float32).ctypes.data_as(vp), b"device"),
            ("host rays", rays.ctypes.data_as(vp), vp(out.data_ptr()), b"device"),
        ]
        for label, a, b, word in table:
            assert lib.rt_trace_hits_device(t._ctx, a, 8, None, b) == -2, label
            assert word in lib.rt_last_error(t._ctx), (label, lib.rt_last_error(t._ctx))
        assert t.hits_info()["calls"] == 3 and bool((out == 7.0).all())
    print("hits device entry ok")


if __name__ == "__main__":
    main()
