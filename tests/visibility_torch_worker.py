"""Child process of tests/test_gpu_visibility.py: rt_visibility_device on torch tensors gives the host entry's bits in all three modes,
on torch's default stream and on a stream of its own; a misaligned pointer and host memory are refused; rt_visibility_info counts the
calls.  torch is imported before the library is loaded (torch brings its own HIP runtime; the library then uses it), so it runs in a
fresh process."""
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
    lib = rtx.load_library()
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    rng = np.random.default_rng(13)
    lo, hi = tr["posA"].min(0), tr["posA"].max(0)
    n = 150
    pts = np.zeros(n, rtx.RAY)
    pts["origin"] = lo - (hi - lo) * 0.25 + rng.random((n, 3)) * 1.5 * (hi - lo)
    nrm = rng.standard_normal((n, 3))
    pts["direction"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    pts["tMax"] = 6.0                                            # (a finite reach: the distance moments stay finite)
    pts["tMax"][::9] = 0.0
    pts["tMax"][1::9] = 3.0
    pts["origin"][5] *= np.float32(1e4)                          # the device entry measures the origin bound itself
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        t.set_option("visibility_slice", 70)                     # three launches per call
        calls = 0
        for mode, shape in ((0, (n, 4)), (1, (n, 12)), (2, (n, 4))):
            want = t.visibility(pts, 5, seed=3, first_index=40, mode=mode)
            calls += 1
            info = t.visibility_info()
            assert info["calls"] == calls and info["samples"] == 5 and info["lastSampleLanes"] == 4 and info["mode"] == mode, info
            assert info["lastKernelMs"] > 0 and info["totalKernelMs"] >= info["lastKernelMs"], info
            assert want.shape == shape and (want[::9] == 0).all() and len(np.unique(want, axis=0)) > 3
            dev = torch.from_numpy(pts.view(np.float32).reshape(-1, 8).copy()).cuda()
            got = t.visibility_device(dev, 5, seed=3, first_index=40, mode=mode)
            calls += 1
            assert tuple(got.shape) == shape and got.dtype == torch.float32 and got.is_cuda
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"default stream, mode {mode}"
            after = t.visibility_info()
            assert after["calls"] == calls and after["lastKernelMs"] == info["lastKernelMs"] and after["totalKernelMs"] == info["totalKernelMs"], after
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                d2 = dev * 1.0                                   # written on the side stream, read by the query on it
                got2 = t.visibility(d2, 5, seed=3, first_index=40, mode=mode).cpu()
            calls += 1
            assert np.array_equal(got2.numpy().view(np.uint32), want.view(np.uint32)), f"side stream, mode {mode}"
        # the manager's method reaches the same entry with a tensor (it sets params first)
        mgr.backend = t
        got3 = mgr.Visibility(dev, 5, seed=3, firstIndex=40, mode=2)
        calls += 1
        assert np.array_equal(got3.cpu().numpy().view(np.uint32), want.view(np.uint32)), "Visibility(tensor)"
        # refusals: a misaligned device pointer (points, then out), host memory
        q = np.zeros((), rtx.VISIBILITY_PARAMS)
        q["samples"] = 5
        qp, vp = q.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p
        out = torch.full((n, 4), 7.0, dtype=torch.float32, device=dev.device)
        torch.cuda.synchronize()
        assert lib.rt_visibility_device(t._ctx, vp(dev.data_ptr() + 4), 8, qp, vp(out.data_ptr())) == -2
        assert b"aligned" in lib.rt_last_error(t._ctx)
        assert lib.rt_visibility_device(t._ctx, vp(dev.data_ptr()), 8, qp, vp(out.data_ptr() + 8)) == -2
        host = np.zeros((8, 4), np.float32)
        assert lib.rt_visibility_device(t._ctx, vp(dev.data_ptr()), 8, qp, host.ctypes.data_as(vp)) == -2
        assert b"device" in lib.rt_last_error(t._ctx)
        assert lib.rt_visibility_device(t._ctx, pts.ctypes.data_as(vp), 8, qp, vp(out.data_ptr())) == -2
        assert t.visibility_info()["calls"] == calls and bool((out == 7.0).all())
    print("visibility device entry ok")


if __name__ == "__main__":
    main()
