"""Child process of tests/test_gpu_device_geometry.py: the torch door.  A float32 (n, 18) CUDA tensor uploaded with
Tracer.upload_triangles_device gives the bits of the host upload; six steps of displacement computed on the device are updated in place and
match a fresh context given the same triangles from host; a tensor overwritten right after the call, on the stream of the call, does not
reach the scene; a tensor with the option at 0 is refused in Python; MultiTracer takes a tensor.  torch is imported before the library is
loaded (torch brings its own HIP runtime; the library then uses it), so this runs in a fresh process of its own."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def as_tensor(tris):
    return torch.from_numpy(np.ascontiguousarray(tris).view(np.float32).reshape(-1, 18).copy()).cuda()


def as_triangles(rtx, tensor):
    return tensor.cpu().numpy().reshape(-1).view(rtx.TRIANGLE).copy()


def displace_on_device(x, step):
    """a smooth field over the corners (columns 0..8 of a triangle record), computed by torch on the device"""
    p = x[:, :9].reshape(-1, 3, 3)
    d = torch.stack([torch.sin(p[..., 1] * 1.3 + step), torch.cos(p[..., 0] * 0.7 + 0.5 * step), torch.sin(p[..., 2] + p[..., 0] + step)], -1)
    out = x.clone()
    out[:, :9] = (p + 0.1 * d).reshape(-1, 9)
    return out


def main():
    import rtx_pkg
    rtx = rtx_pkg.load()
    from device_geometry_helpers import assert_same, fresh_snapshot, query_rays, small_scene, snapshot
    from test_gpu_bvh_audit import audit_tracer

    scene = small_scene(rtx, 257)
    params, spheres, tris, infos = scene
    rays = query_rays(rtx, params, spheres, tris)

    # ---- the same scene through both doors, then six steps of on-device displacement
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, meshinfo=infos)
        x = as_tensor(tris)
        t.upload_triangles_device(x)
        assert_same(snapshot(rtx, t, params, rays), fresh_snapshot(rtx, scene, rays), "tensor against host upload")
        assert t.stats()["bvhBuilds"] == 1
        for step in range(1, 7):
            x = displace_on_device(x, step)
            t.upload_triangles_device(x)
            now = as_triangles(rtx, x)
            full = step in (1, 6)
            assert_same(snapshot(rtx, t, params, rays, frames=full), fresh_snapshot(rtx, (params, spheres, now, infos), rays, frames=full),
                        f"on-device displacement, step {step}")
            st = t.stats()
            assert (st["bvhBuilds"], st["bvhRebuilds"], st["numTriangles"]) == (1, 0, 257), (step, st)
            audit_tracer(t, now, f"on-device displacement, step {step}", refitted=True)

        # ---- order and ownership: written on a side stream, uploaded on it, overwritten on it right after the call
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            y = displace_on_device(x, 7)                         # (the upload must see this write ...)
            keep = y.clone()
            t.upload_triangles_device(y)
            y.fill_(float("nan"))                                # (... and not this one)
        got = snapshot(rtx, t, params, rays)
        side.synchronize()
        assert_same(got, fresh_snapshot(rtx, (params, spheres, as_triangles(rtx, keep), infos), rays), "a tensor overwritten after the call")
        assert t.stats()["bvhBuilds"] == 1

        # ---- a tensor while the option is 0: refused in Python, nothing changes
        t.set_option("kernel", 1)
        t.reset_accum(); t.render(0, 1)
        image, st0 = t.read_accum().tobytes(), t.stats()
        t.set_option("device_geometry", 0)
        try:
            t.upload_triangles_device(x)
        except rtx.RtError as e:
            assert "device_geometry is 0" in str(e)
        else:
            raise AssertionError("a tensor was accepted with device_geometry = 0")
        assert t.read_accum().tobytes() == image and t.stats() == st0
        for bad in (x[:, :17], x.double(), x.t()):
            try:
                t.upload_triangles_device(bad)
            except ValueError:
                pass
            else:
                raise AssertionError(f"accepted a tensor of {bad.dtype} {tuple(bad.shape)}")

    # ---- rt_multi takes a tensor
    with rtx.Tracer(0) as t:
        t.set_option("device_bvh", 1); t.set_option("kernel", 1)
        t.set_params(params)
        t.upload(spheres=spheres, triangles=as_triangles(rtx, x), meshinfo=infos)
        t.render(0, 2)
        want = t.read_accum().tobytes()
    with rtx.MultiTracer([0, 0]) as m:
        m.set_option("kernel", 1)
        m.set_params(params)
        m.upload(spheres=spheres, meshinfo=infos)
        m.upload_triangles_device(x)
        m.render(0, 2)
        assert m.read_accum().tobytes() == want, "rt_multi from a tensor"
    print("device geometry ok")


if __name__ == "__main__":
    main()
