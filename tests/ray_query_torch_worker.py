"""Child process of tests/test_gpu_ray_query.py: the device entries on torch tensors give the host entries' bits, on torch's default stream
and on a stream of its own, and switching the context's stream is ordered.  torch is imported before the library is loaded (torch brings
its own HIP runtime; the library then uses it), so it runs in a fresh process of its own."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    rng = np.random.default_rng(13)
    lo, hi = tr["posA"].min(0), tr["posA"].max(0)
    rays = np.zeros(3000, rtx.RAY)
    rays["origin"] = lo - (hi - lo) + rng.random((3000, 3)) * 3 * (hi - lo)
    rays["direction"] = rng.standard_normal((3000, 3))
    rays["tMax"] = np.inf
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        want, want_occ = t.trace_rays(rays), t.occluded(rays)
        assert (want["kind"] != 0).any()
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        got = t.trace_rays(dev)
        assert got.shape == (3000, 16) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32).reshape(-1, 16)), "default stream: hits"
        assert np.array_equal(t.occluded(dev).cpu().numpy(), want_occ), "default stream: occlusion"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d2 = dev * 1.0                                       # written on the side stream, read by the queries on it
            got2, occ2 = t.trace_rays(d2).cpu(), t.occluded(d2).cpu()
        assert np.array_equal(got2.numpy().view(np.uint32), want.view(np.uint32).reshape(-1, 16)), "side stream: hits"
        assert np.array_equal(occ2.numpy(), want_occ), "side stream: occlusion"
        # rt_set_stream's switch is ordered: work left on the outgoing stream (here a long sleep kernel where a device query could be)
        # completes before anything the context enqueues afterwards on its own stream
        t.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            torch.cuda._sleep(100_000_000)
        t.set_stream(0)
        t.trace_rays(rays[:16])                                  # host entry: returns once the context's own stream has drained
        assert side.query(), "the context's own stream did not wait for the stream it switched away from"
    print("device entries ok")


if __name__ == "__main__":
    main()
