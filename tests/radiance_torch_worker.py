"""Child process of tests/test_gpu_radiance.py: rt_trace_radiance_device on torch tensors gives the host entry's bits, on torch's default
stream and on a stream of its own; a misaligned pointer and host memory are refused; rt_radiance_info counts the calls.  torch is imported
before the library is loaded (torch brings its own HIP runtime; the library then uses it), so it runs in a fresh process of its own."""
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
    n = 1500
    rays = np.zeros(n, rtx.RAY)
    rays["origin"] = lo - (hi - lo) + rng.random((n, 3)) * 3 * (hi - lo)
    rays["direction"] = rng.standard_normal((n, 3))
    rays["tMax"] = np.inf
    rays["tMax"][::9] = 0.0
    rays["origin"][5] *= np.float32(1e4)                         # the device entry measures the origin bound itself
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        t.set_option("radiance_slice", 700)                      # three launches per call
        want = t.trace_radiance(rays, 5, seed=3, first_index=40)
        info = t.radiance_info()
        assert info["calls"] == 1 and info["samples"] == 5 and info["lastSampleLanes"] == 4 and info["lastKernelMs"] > 0, info
        assert info["totalKernelMs"] == info["lastKernelMs"]
        assert (want[:, 3] == 1).any() and (want[::9] == 0).all() and len(np.unique(want[:, :3], axis=0)) > 100
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        got = t.trace_radiance(dev, 5, seed=3, first_index=40)
        assert got.shape == (n, 4) and got.dtype == torch.float32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), "default stream"
        after = t.radiance_info()
        assert after["calls"] == 2 and after["lastKernelMs"] == info["lastKernelMs"] and after["totalKernelMs"] == info["totalKernelMs"], after
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d2 = dev * 1.0                                       # written on the side stream, read by the query on it
            got2 = t.trace_radiance(d2, 5, seed=3, first_index=40).cpu()
        assert np.array_equal(got2.numpy().view(np.uint32), want.view(np.uint32)), "side stream"
        # the manager's tensor method reaches the same entry
        mgr.backend = t
        got3 = mgr.TraceRadianceTensor(dev, 5, seed=3, firstIndex=40)
        assert np.array_equal(got3.cpu().numpy().view(np.uint32), want.view(np.uint32)), "TraceRadianceTensor"
        # refusals: a misaligned device pointer (rays, then rgba), host memory
        q = np.zeros((), rtx.RADIANCE_PARAMS)
        q["samples"] = 5
        qp, vp = q.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p
        out = torch.empty((n, 4), dtype=torch.float32, device=dev.device)
        torch.cuda.synchronize()
        calls = t.radiance_info()["calls"]
        assert lib.rt_trace_radiance_device(t._ctx, vp(dev.data_ptr() + 4), 8, qp, vp(out.data_ptr())) == -2
        assert b"aligned" in lib.rt_last_error(t._ctx)
        assert lib.rt_trace_radiance_device(t._ctx, vp(dev.data_ptr()), 8, qp, vp(out.data_ptr() + 8)) == -2
        host = np.zeros((8, 4), np.float32)
        assert lib.rt_trace_radiance_device(t._ctx, vp(dev.data_ptr()), 8, qp, host.ctypes.data_as(vp)) == -2
        assert b"device" in lib.rt_last_error(t._ctx)
        assert lib.rt_trace_radiance_device(t._ctx, rays.ctypes.data_as(vp), 8, qp, vp(out.data_ptr())) == -2
        assert t.radiance_info()["calls"] == calls
    print("radiance device entry ok")


if __name__ == "__main__":
    main()
