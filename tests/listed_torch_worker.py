"""Child process of tests/test_gpu_nearest.py, test_gpu_overlap.py and test_gpu_capsule.py: listed_torch_worker.py <family>.
rt_closest_points_device with the family's options on torch tensors gives the checker's bits as an (n, K, 16) tensor, on torch's default
stream and on a stream of its own, with and without the counting kernel; the family's Python helpers (nearest.py, overlap.py,
capsule.py) take tensors, and for capsules the device path's origin bound sees both endpoints; at the defaults the tensor is the
closest-point call's again.  torch is imported before the library is loaded (torch brings its own HIP runtime; the library then uses
it), so it runs in a fresh process."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def as_records(rtx, t, k):
    return t.cpu().numpy().view(rtx.CLOSEST).reshape(-1, k)


# ---- per family: the batch, and the tensor-helper checks (form, want: a (K, all) of the loop and the checker's answer, or None after it) ----
def nearest_batch(rtx, s, tr, mi):
    import closest_check as cc
    import nearest_check as nc
    rng = np.random.default_rng(13)
    lo, hi = tr["posA"].min(0), tr["posA"].max(0)
    pts = cc.points_of(rtx, lo - (hi - lo) * 0.25 + rng.random((150, 3)) * 1.5 * (hi - lo))
    pts["tMax"][::9] = 0.0
    pts["tMax"][1::9] = 0.75
    pts["origin"][5] *= np.float32(1e4)                          # the device entry measures the origin bound itself
    return np.concatenate([nc.vertex_tie_points(rtx, s, tr, mi, 40), pts])


def nearest_helpers(rtx, t, dev, pts, s, tr, mi, form, want):
    import nearest_check as nc
    n = len(pts)
    if form:
        k, count_all = form
        got3 = rtx.nearest.nearest_k(t, dev, k, count_all=bool(count_all))
        assert tuple(got3.shape) == (n, k, 16)
        nc.assert_same_records(rtx, as_records(rtx, got3, k), want, f"nearest_k(tensor), K {k} all {count_all}")
        return
    R = np.float32(0.75)
    counts = rtx.nearest.overlap_count(t, dev, float(R))
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (n,)
    q = pts.copy()
    q["tMax"] = R
    want = nc.oracle_nearest(rtx, s, tr, mi, q, 1, 1)["_reserved"][:, 0, 0]
    assert np.array_equal(counts.cpu().numpy(), want) and want.max() > 1


def overlap_batch(rtx, s, tr, mi):
    import overlap_check as oc
    from test_gpu_closest import batch_of
    return oc.batch_of(rtx, s, tr, mi, batch_of(rtx, s, tr, mi)[::3], per_kind=12)


def overlap_helpers(rtx, t, dev, boxes, s, tr, mi, form, want):
    import overlap_check as oc
    n = len(boxes)
    gate = boxes.copy()
    gate["tMax"] = 1.0                                           # (the helper's gate is always open)
    if form:
        k, count_all = form
        got3 = rtx.overlap.overlap_box(t, dev[:, 0:3].contiguous(), dev[:, 4:7].contiguous(), k, count_all=bool(count_all))
        assert tuple(got3.shape) == (n, k, 16)
        oc.assert_same_records(rtx, as_records(rtx, got3, k), oc.oracle_overlap(rtx, s, tr, mi, gate, k, count_all), f"overlap_box(tensor), K {k} all {count_all}")
        return
    any_ = rtx.overlap.check_box(t, dev[:, 0:3].contiguous(), dev[:, 4:7].contiguous())
    assert any_.dtype == torch.uint8 and tuple(any_.shape) == (n,)
    want = (oc.counts(oc.oracle_overlap(rtx, s, tr, mi, gate, 1, 0))[:, 0] != 0)
    assert np.array_equal(any_.cpu().numpy(), want.astype(np.uint8)) and 0 < want.sum() < n


def capsule_batch(rtx, s, tr, mi):
    import capsule_check as kc
    from test_gpu_closest import batch_of
    return kc.batch_of(rtx, s, tr, mi, batch_of(rtx, s, tr, mi)[::3], per_kind=12)


def capsule_helpers(rtx, t, dev, segs, s, tr, mi, form, want):
    import capsule_check as kc
    if form:
        return
    # the helpers on tensors (finite inputs: the helper forms d = p1 - p0 again)
    ok = np.isfinite(segs["origin"]).all(1) & np.isfinite(segs["direction"]).all(1) & (np.abs(segs["origin"]) < 1e30).all(1)
    p0 = dev[torch.from_numpy(ok).cuda(), 0:3].contiguous()
    p1 = p0 + dev[torch.from_numpy(ok).cuda(), 4:7]
    again_segs = kc.segments_of(rtx, p0.cpu().numpy(), p1.cpu().numpy(), 1.5)
    got3 = rtx.capsule.overlap_capsule(t, p0, p1, 1.5, 4, count_all=True)
    assert tuple(got3.shape) == (int(ok.sum()), 4, 16)
    kc.assert_same_records(rtx, as_records(rtx, got3, 4), kc.oracle_capsule(rtx, s, tr, mi, again_segs, 4, 1), "overlap_capsule(tensor)")
    any_ = rtx.capsule.check_capsule(t, p0, p1, 1.5)
    want = kc.counts(kc.oracle_capsule(rtx, s, tr, mi, again_segs, 1, 0))[:, 0] != 0
    assert any_.dtype == torch.uint8 and np.array_equal(any_.cpu().numpy(), want.astype(np.uint8)) and 0 < want.sum() < len(want)
    rec, par = rtx.capsule.closest_to_segment(t, p0, p1)
    again_segs["tMax"] = np.inf
    want = kc.oracle_capsule(rtx, s, tr, mi, again_segs, 1, 0)
    kc.assert_same_records(rtx, as_records(rtx, rec, 1), want, "closest_to_segment(tensor)")
    assert np.array_equal(par.cpu().numpy().view(np.uint32), kc.params(want)[:, 0].view(np.uint32))
    # the device path's origin bound: P0 near the scene, P1 1e8 away (beyond everything the batch above reached) widens the padding once
    far = kc.segments_of(rtx, again_segs["origin"][:130], d=np.repeat(np.float32([[1e8, 0, -7e7]]), 130, 0), radius=2.0)
    before = t.stats()["bvhRepads"]
    fdev = torch.from_numpy(far.view(np.float32).reshape(-1, 8).copy()).cuda()
    t.closest_points(fdev)                                       # as points: nothing moves
    assert t.stats()["bvhRepads"] == before
    got4 = rtx.capsule.overlap_capsule(t, fdev[:, 0:3].contiguous(), fdev[:, 0:3] + fdev[:, 4:7], 2.0, 8)
    far = kc.segments_of(rtx, far["origin"], far["origin"] + far["direction"], 2.0)
    kc.assert_same_records(rtx, as_records(rtx, got4, 8), kc.oracle_capsule(rtx, s, tr, mi, far, 8, 0), "P1 far away, device entry")
    assert t.stats()["bvhRepads"] == before + 1


# family -> (its batch, lastPrimTests' lower bound from (inputs, spheres, the checker's answer), its helper checks)
WORK = {"nearest": (nearest_batch, lambda pts, s, want: int((pts["tMax"] > 0).sum()) * len(s), nearest_helpers),
        "overlap": (overlap_batch, lambda boxes, s, want: int(want["_reserved"][:, 0, 0].sum()), overlap_helpers),
        "capsule": (capsule_batch, lambda segs, s, want: int(want["_reserved"][:, 0, 0].sum()), capsule_helpers)}


def main(family):
    import rtx_pkg
    rtx = rtx_pkg.load()
    import closest_check as cc
    from listed_gpu import FAMILIES
    fam = FAMILIES[family]
    batch, tests_at_least, helpers = WORK[family]
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    inputs = batch(rtx, s, tr, mi)
    n = len(inputs)
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)           # (no params: the call needs none)
        t.set_option("closest_slice", 70)                        # several launches per call
        dev = torch.from_numpy(inputs.view(np.float32).reshape(-1, 8).copy()).cuda()
        default = t.closest_points(dev)
        assert tuple(default.shape) == (n, 16)
        cc.assert_same_records(rtx, as_records(rtx, default, 1)[:, 0], cc.oracle_closest(rtx, s, tr, mi, inputs), "defaults before")
        for k, count_all in fam.check.FORMS:
            want = fam.oracle(rtx, s, tr, mi, inputs, k, count_all)
            if fam.option:
                t.set_option(fam.option, 1)
            t.set_option("closest_k", k)
            t.set_option("closest_all", count_all)
            got = t.closest_points_device(dev)
            assert (tuple(got.shape) == ((n, k, 16) if k > 1 else (n, 16))) and got.dtype == torch.float32 and got.is_cuda
            fam.check.assert_same_records(rtx, as_records(rtx, got, k), want, f"default stream, K {k} all {count_all}")
            t.set_option("closest_count", 1)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                d2 = dev * 1.0                                   # written on the side stream, read by the query on it
                got2 = t.closest_points(d2)
                counted = t.closest_info()                       # (waits for the stream once, for the counts)
                got2 = got2.cpu()
            fam.check.assert_same_records(rtx, as_records(rtx, got2, k), want, f"side stream, counting kernel, K {k} all {count_all}")
            assert counted["lastPrimTests"] >= tests_at_least(inputs, s, want) and counted["lastNodeSteps"] > 0, counted
            t.set_option("closest_count", 0)
            if fam.option:
                t.set_option(fam.option, 0)
            t.set_option("closest_k", 1)
            t.set_option("closest_all", 0)
            helpers(rtx, t, dev, inputs, s, tr, mi, (k, count_all), want)
        helpers(rtx, t, dev, inputs, s, tr, mi, None, None)
        again = t.closest_points(dev)                            # the helpers put the defaults back
        assert tuple(again.shape) == (n, 16) and torch.equal(again.view(torch.int32), default.view(torch.int32))
    print(f"{family} device entry ok")


if __name__ == "__main__":
    main(sys.argv[1])
