"""On-device geometry pipeline (rt_upload_local_meshes / rt_set_mesh_transforms): the GPU's world-space triangles and
chunk bounds equal the host marshal's bytes (RayTracedMesh.cs:56-94 restated in host.py), and images rendered through it —
including after a BVH *refit* for moved meshes — are bit-identical to uploading host-transformed buffers."""
import os

import numpy as np
import pytest

from bvh_audit import random_pose
from test_gpu_parity import assert_bitwise, run_gpu

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def upload_local(tracer, mgr):
    params, spheres, _, _ = mgr.build_buffers()
    tracer.set_rows(0, int(params["height"]))
    tracer.set_params(params)
    tracer.upload(spheres=spheres)
    tracer.upload_local_meshes(*mgr.build_local_buffers(), len(mgr.meshes))
    tracer.set_mesh_transforms(mgr.build_transforms())
    return params


def bytes_equal(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("scene", ["mesh_test", "Knight", "config3"])
def test_device_world_geometry_equals_host_marshal(rtx, tracer, scene):
    from rtx_amd import unity_scene
    if scene == "mesh_test":
        mgr = rtx.scenes.mesh_test_scene(64, 48)
    elif scene == "Knight":
        mgr = unity_scene.load_scene_npz(os.path.join(GOLDEN, "scenes", "Knight.npz"), 64, 36)
    else:
        mgr = rtx.scenes.config3(64, 36)
    _, _, tris, infos = mgr.build_buffers()
    upload_local(tracer, mgr)
    dtris, dinfos = tracer.read_world_geometry()
    assert len(dtris) == len(tris) and len(dinfos) == len(infos)
    for k in tris.dtype.names:
        assert bytes_equal(dtris[k], tris[k]), f"{scene}: triangles.{k} differ"
    for k in ("firstTriangleIndex", "numTriangles", "boundsMin", "boundsMax"):
        assert bytes_equal(dinfos[k], infos[k]), f"{scene}: meshinfo.{k} differ"
    assert bytes_equal(dinfos["material"], infos["material"])
    print(f"{scene}: {len(tris)} triangles, device geometry pass {tracer.stats()['lastGeometryMs']:.3f} ms")


@pytest.mark.parametrize("mode", [0, 1])
def test_device_pipeline_image_equals_host_path(rtx, tracer, mode):
    mgr = rtx.scenes.mesh_test_scene(96, 64)
    mgr.intersectMode = mode
    want, want_last = run_gpu(tracer, mgr.build_buffers(), 1, 2, mode=mode)
    upload_local(tracer, mgr)
    tracer.reset_accum()
    tracer.render(1, 2)
    assert_bitwise(tracer.read_last_frame(), want_last, f"device geometry, mode {mode}, last frame")
    assert_bitwise(tracer.read_accum(), want, f"device geometry, mode {mode}, accum")


def test_refit_after_moving_meshes_equals_fresh_upload(rtx, tracer):
    """Animate: move / rotate / rescale the meshes -> only new transforms are sent, the BVH is refitted on the device."""
    mgr = rtx.scenes.mesh_test_scene(96, 64)
    upload_local(tracer, mgr)
    tracer.reset_accum()
    tracer.render(0, 1)
    nodes_before = tracer.stats()["numBvhNodes"]
    h = rtx.host
    for step in range(2):
        for i, mesh in enumerate(mgr.meshes[2:]):
            a = 0.4 * (i + 1) + 0.7 * step
            q = h.quat_mul((0.0, np.sin(a / 2), 0.0, np.cos(a / 2)), mesh.transform.rotation)
            mesh.transform = h.Transform(position=mesh.transform.position + np.float32([0.3 * step, 0.1 * i, -0.2]),
                                         rotation=q, lossyScale=mesh.transform.lossyScale * np.float32(1.1))
        tracer.set_mesh_transforms(mgr.build_transforms())          # 40 B per mesh
        tracer.reset_accum()
        tracer.render(3, 2)
        got, got_last = tracer.read_accum(), tracer.read_last_frame()
        assert tracer.stats()["numBvhNodes"] == nodes_before        # topology kept: refit, not rebuild
        dtris, dinfos = tracer.read_world_geometry()
        _, _, tris, infos = mgr.build_buffers()
        assert bytes_equal(dtris["posB"], tris["posB"]) and bytes_equal(dinfos["boundsMax"], infos["boundsMax"])
        want, want_last = run_gpu(tracer, mgr.build_buffers(), 3, 2)   # fresh host-transformed upload + BVH build
        assert_bitwise(got_last, want_last, f"refit step {step}, last frame")
        assert_bitwise(got, want, f"refit step {step}, accum")
        if step == 0:                                                # (run_gpu switched the context to the world path)
            upload_local(tracer, mgr)
            tracer.render(0, 1)
            nodes_before = tracer.stats()["numBvhNodes"]


def test_manager_device_geometry_flag(rtx, tracer):
    """RayTracingManager.OnRenderImage with deviceGeometry=True == the default host-marshal path."""
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    want, _ = run_gpu(tracer, mgr.build_buffers(), 0, 2)
    mgr2 = rtx.scenes.mesh_test_scene(64, 48)
    mgr2.backend, mgr2.deviceGeometry = tracer, True
    mgr2.Start()
    got = mgr2.OnRenderImage(frames=2)
    assert_bitwise(got, want, "manager with deviceGeometry")


@pytest.mark.parametrize("seed", range(10))
def test_random_transforms_device_geometry_equals_host_marshal(rtx, tracer, seed):
    """Random poses per mesh — arbitrary unit quaternions (and a slightly non-unit one), non-uniform, negative and zero scales,
    translations up to 1e3 — through the device pipeline: world triangles and chunk bounds equal the host marshal's bytes,
    and the image equals the host path's (the second pose set goes through the BVH refit)."""
    rng = np.random.default_rng(500 + seed)
    mgr = rtx.scenes.mesh_test_scene(64, 48)

    def pose():
        random_pose(rtx, mgr, rng, seed)

    pose()
    upload_local(tracer, mgr)
    for round_ in range(2):
        if round_ == 1:
            pose()
            tracer.set_mesh_transforms(mgr.build_transforms())      # same topology: refit
        _, _, tris, infos = mgr.build_buffers()
        tracer.reset_accum()
        tracer.render(round_, 1)
        got = tracer.read_last_frame()
        dtris, dinfos = tracer.read_world_geometry()
        for k in tris.dtype.names:
            assert bytes_equal(dtris[k], tris[k]), f"seed {seed} round {round_}: triangles.{k} differ"
        for k in ("boundsMin", "boundsMax"):
            assert bytes_equal(dinfos[k], infos[k]), f"seed {seed} round {round_}: meshinfo.{k} differ"
        _, want = run_gpu(tracer, mgr.build_buffers(), round_, 1, kernel=-1)
        assert_bitwise(got, want, f"seed {seed} round {round_}: image through the device pipeline")
        if round_ == 0:
            upload_local(tracer, mgr)                                # back to the local-mesh path for the refit round


# ---- chunk boxes over NaN vertices: the reference's order and comparison --------------------------------------------

def test_chunk_bounds_follow_the_reference_rule_on_nan_vertices(rtx):
    """k_chunk_bounds on the hand cases of tests/test_dynamic_fuzz_cpu.py — one chunk per case, identity pose, so a NaN vertex is NaN on
    every axis: a NaN coordinate replaces the running bound and the next vertex replaces the NaN (fminf / fmaxf would skip it)."""
    import dynamic_fuzz as df
    from test_dynamic_fuzz_cpu import HAND
    n = sum(len(seq) // 3 for _, seq, _, _ in HAND)
    tris, chunks = np.zeros(n, rtx.TRIANGLE), np.zeros(len(HAND), rtx._cabi.LOCAL_CHUNK)
    at = 0
    for c, (_, seq, _, _) in enumerate(HAND):
        pts = np.repeat(np.asarray(seq, np.float32)[:, None], 3, 1)
        k = len(seq) // 3
        tris["posA"][at:at + k], tris["posB"][at:at + k], tris["posC"][at:at + k] = pts[0::3], pts[1::3], pts[2::3]
        chunks[c]["firstTriangleIndex"], chunks[c]["numTriangles"] = at, k
        at += k
    xf = np.zeros(1, rtx._cabi.MESH_TRANSFORM)
    xf["rotation"], xf["lossyScale"] = (0, 0, 0, 1), (1, 1, 1)
    params = rtx.scenes.mesh_test_scene(16, 8).build_buffers()[0]
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload_local_meshes(tris, chunks, 1)
        t.set_mesh_transforms(xf)
        for round_ in range(2):                            # the build's pass, then a refit's
            if round_:                                     # away and back, a frame in each pose, so that the pass runs again on a standing tree
                t.render(0, 1)
                away = xf.copy(); away["position"] = (1.0, 2.0, 4.0)
                t.set_mesh_transforms(away)
                t.render(0, 1)
                assert t.read_world_geometry()[1]["boundsMin"].tobytes() != infos["boundsMin"].tobytes(), "the pose did not move the boxes"
                builds = t.stats()["bvhBuilds"]
                t.set_mesh_transforms(xf)
                t.render(0, 1)
                assert t.stats()["bvhBuilds"] == builds, "round 1 is a refit"
            _, infos = t.read_world_geometry()
            for c, (what, _, lo, hi) in enumerate(HAND):
                want = df.bounds_round_trip(np.float32([lo] * 3), np.float32([hi] * 3))
                for got, w, name in ((infos[c]["boundsMin"], want[0], "boundsMin"), (infos[c]["boundsMax"], want[1], "boundsMax")):
                    assert got.tobytes() == w.tobytes() or (np.isnan(got).all() and np.isnan(w).all()), f"{what} (round {round_}): {name} {got}, want {w}"


@pytest.mark.parametrize("hostile", ["quaternion of norm 3", "quaternion of norm 3 on a mesh scaled 1e18", "infinite local vertex"])
def test_refit_padding_covers_a_long_quaternion_and_an_infinite_vertex(rtx, hostile):
    """the two bounds of the local door's padding that reading alone left open (local_scene_magnitude took p + 1.01 |s| radius, and a
    quaternion of norm 3 makes the mesh up to seventeen times larger; radius runs over |p| with infinity in it): two meshes stand, one
    is posed again, and the refitted tree (rebuild_percent 0: never rebuilt) passes the audit whole, padding check included
    (refitted=True), over the reference's world triangles.  The 1e18 case is what tests/dynamic_fuzz.py seeds 36 and 96 showed at
    step 6: the faces near zero were 4 to 7 times short of the 2e-6 G a build gives, because G took the quaternion for a unit one;
    local_scene_magnitude bounds the mesh by (|1 - |q|^2| + |q|^2) |s| radius since."""
    import dynamic_fuzz as df
    from bvh_audit import awkward_triangles
    from test_gpu_bvh_audit import audit_tracer
    local, _ = awkward_triangles(rtx, 65)
    if hostile == "infinite local vertex":
        local["posC"][7, 1] = np.inf
        local["posB"][40, 0] = -np.inf
    chunks = np.zeros(2, rtx._cabi.LOCAL_CHUNK)
    chunks["firstTriangleIndex"], chunks["numTriangles"], chunks["meshIndex"] = (0, 33), (33, 32), (0, 1)
    xf = np.zeros(2, rtx._cabi.MESH_TRANSFORM)
    xf["rotation"], xf["lossyScale"], xf["position"] = (0, 0, 0, 1), (1, 1, 1), ((0, 0, 0), (3, 0, 1))
    if "1e18" in hostile:
        xf["lossyScale"][1] = 1e18
    params = rtx.scenes.mesh_test_scene(16, 8).build_buffers()[0]
    with rtx.Tracer(0) as t:
        t.set_option("device_bvh", 1)
        t.set_option("rebuild_percent", 0)
        t.set_params(params)
        t.upload_local_meshes(local, chunks, 2)
        t.set_mesh_transforms(xf)
        t.render(0, 1)
        builds = t.stats()["bvhBuilds"]
        again = xf.copy()
        q = np.float64([0.3, -0.5, 0.4, 0.7])
        again["rotation"][1] = q / np.linalg.norm(q) * (1.0 if hostile == "infinite local vertex" else 3.0)
        again["position"][1] = (2.5, 0.5, 1.0)
        t.set_mesh_transforms(again)
        t.render(1, 1)
        assert t.stats()["bvhBuilds"] == builds, "a pose on a standing tree refits"
        world, _ = df.world_from_local(rtx, local, chunks, again)
        audit_tracer(t, world, f"{hostile}, refitted", refitted=True)


def test_area_rule_rebuilds_a_tree_whose_built_area_is_5e36(rtx):
    """a standing tree whose area at the build is about 5e36 and whose mesh then doubles in size: the refitted area is four times the
    built one and rebuild_percent (200) asks for a rebuild.  The threshold used to be area_at_build * percent / 100, whose product
    overflows float from 1.7e36 on: inf > inf is false, the tree stayed while refitAreaRatio said 4 (tests/dynamic_fuzz.py seed 96
    step 6 reported inf).  Both area rules compare the ratio with percent / 100 since."""
    rng = np.random.default_rng(11)
    local = np.zeros(64, rtx.TRIANGLE)
    for k in ("posA", "posB", "posC"):
        local[k] = rng.uniform(-1, 1, (64, 3))
    chunks = np.zeros(1, rtx._cabi.LOCAL_CHUNK)
    chunks["numTriangles"] = 64
    xf = np.zeros(1, rtx._cabi.MESH_TRANSFORM)
    xf["rotation"], xf["lossyScale"] = (0, 0, 0, 1), (1, 1, 1)
    params = rtx.scenes.mesh_test_scene(16, 8).build_buffers()[0]
    with rtx.Tracer(0) as t:
        t.set_option("device_bvh", 1)
        t.set_params(params)
        t.upload_local_meshes(local, chunks, 1)
        t.set_mesh_transforms(xf)
        t.render(0, 1)
        unit = float(t.stats()["bvhInternalArea"])
        assert 1.0 < unit < 1e4
        scale = np.float32(np.sqrt(5e36 / unit))                # areas go with the square of the scale
        xf["lossyScale"] = scale
        t.upload_local_meshes(local, chunks, 1)                 # a new scene: built in this pose
        t.set_mesh_transforms(xf)
        t.render(0, 1)
        before = t.stats()
        assert 2e36 < before["bvhInternalArea"] < 2e37, before["bvhInternalArea"]
        xf["lossyScale"] = np.float32(2) * scale
        t.set_mesh_transforms(xf)
        t.render(1, 1)
        after = t.stats()
        assert 3.0 < after["refitAreaRatio"] < 5.0, after["refitAreaRatio"]
        assert (after["bvhBuilds"] - before["bvhBuilds"], after["bvhRebuilds"] - before["bvhRebuilds"]) == (1, 1)


@pytest.mark.parametrize("kernel", [0, 1])
def test_nan_chunk_box_faces_cut_what_the_reference_cuts(rtx, oracle, tracer, kernel):
    """chunk boxes with a NaN boundsMin component, a NaN boundsMax component and all faces NaN (what a chunk whose last vertex is NaN now
    gets): both kernels equal the oracle, whose tree equals its loop on this scene (tests/test_dynamic_fuzz_cpu.py)"""
    from test_dynamic_fuzz_cpu import nan_box_scene
    b = nan_box_scene(rtx)
    acc, last = run_gpu(tracer, b, 0, 2, kernel=kernel)
    want_acc, want_last, cnt = oracle.render(*b, 0, 2, accel=True)
    assert_bitwise(last, want_last, f"NaN chunk boxes, kernel {kernel}, last frame")
    assert_bitwise(acc, want_acc, f"NaN chunk boxes, kernel {kernel}, accum")
    assert tracer.stats()["rays"] == cnt["rays"]
