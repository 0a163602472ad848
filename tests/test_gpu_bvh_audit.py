"""Every tree the tracer holds, audited whole (tests/bvh_audit.py): read back with rt_read_bvh / rt_read_bvh_order and checked node by node
against the world triangles — topology, leaf ranges and order, triangle-in-box down every path, padding, nesting, the f16 form and the
stack bound — after the device builder (awkward counts, every clustering radius, the treelet option sets, the host-built top), the host
builder (with triangles no chunk addresses), local meshes after upload / refit / the area-triggered rebuild / random poses, re-padding
(a drifting camera, far query origins), a world-space scene uploaded again and again, and one 100,440-triangle tree.  The image shows a
wrong box only to the rays that graze it; the last tests aim a ray at every box face a triangle touches and compare with the oracle.
The neighbouring tests compare the images of these states with the oracle; these render the smallest frame that makes the library build."""
import numpy as np
import pytest

from bvh_audit import (aimed_ray_shares, aimed_rays, assert_clean, audit, awkward_triangles, live_triangles, ragged_chunk_scene,
                       random_pose)
from ray_query_helpers import make_rays, shim      # noqa: F401 (shim is a fixture)
from test_gpu_geometry import upload_local
from test_gpu_ray_query import check_queries, loaded_tracer

pytestmark = pytest.mark.gpu

DEFAULTS = {"device_bvh": -1, "bvh_radius": -16, "bvh_treelets": 6, "bvh_treelet_ratio": 8, "bvh_treelet_first": 1, "bvh_treelet_isolate": 1, "bvh_top": 0}


def audit_tracer(t, tris, what, live=None, refitted=False):
    """the audit of the tree `t` holds over the world triangles `tris` -> (report, stats)"""
    f32, f16 = t.read_bvh()
    st = t.stats()
    assert len(f32) == st["numBvhNodes"]
    rep = audit(f32, f16, t.read_bvh_order(), tris, live=live, max_stack=st["bvhMaxStack"], refitted=refitted,
                exact_stack=bool(st["bvhBuiltOnDevice"]))
    assert_clean(rep, what)
    return rep, st


def build_and_audit(tracer, b, what, live=None, **opts):
    """upload the world-space scene `b`, trace one frame of it — which builds it with the given options — and audit the tree (before
    the options go back to their defaults: setting one asks for a new build)"""
    params, spheres, tris, infos = b
    for k, v in opts.items():
        tracer.set_option(k, v)
    try:
        tracer.set_option("kernel", 1)
        tracer.set_rows(0, int(params["height"]))
        tracer.set_params(params)
        tracer.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        tracer.reset_accum()
        tracer.render(0, 1)
        return audit_tracer(tracer, tris, what, live=live)
    finally:
        for k in opts:
            tracer.set_option(k, DEFAULTS[k])


@pytest.fixture(scope="module")
def mesh_scene(rtx):
    m = rtx.scenes.mesh_test_scene(16, 8)
    m.numRaysPerPixel = 1
    return m.build_buffers()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 47, 513, 1025])
def test_device_builder_awkward_triangle_counts(rtx, tracer, mesh_scene, n):
    tris, infos = awkward_triangles(rtx, n)
    rep, st = build_and_audit(tracer, (mesh_scene[0], mesh_scene[1], tris, infos), f"device builder, {n} triangles", device_bvh=1)
    assert st["bvhBuiltOnDevice"] == 1 and rep.n_triangles == n


@pytest.mark.parametrize("radius", [1, 8, -16, 64])
def test_device_builder_every_clustering_radius(tracer, mesh_scene, radius):
    rep, st = build_and_audit(tracer, mesh_scene, f"device builder, radius {radius}", device_bvh=1, bvh_radius=radius)
    assert st["bvhBuiltOnDevice"] == 1 and rep.n_triangles == len(mesh_scene[2])


@pytest.mark.parametrize("passes,ratio,first,isolate", [(1, 8, 1, 1), (2, 4, 1, 0), (3, 8, 2, 1), (16, 2, 1, 1), (6, 64, 1, 1)])
def test_device_builder_treelet_option_sets_and_the_host_built_top(tracer, mesh_scene, passes, ratio, first, isolate):
    for top in (0, 7, 1024):
        _, st = build_and_audit(tracer, mesh_scene, f"treelets {passes} x{ratio} first {first} iso {isolate} top {top}", device_bvh=1, bvh_treelets=passes,
                                bvh_treelet_ratio=ratio, bvh_treelet_first=first, bvh_treelet_isolate=isolate, bvh_top=top)
        assert st["bvhBuiltOnDevice"] == 1


def test_host_builder_through_the_tracer(tracer, mesh_scene):
    rep, st = build_and_audit(tracer, mesh_scene, "host builder, mesh-test scene", device_bvh=0)
    assert st["bvhBuiltOnDevice"] == 0 and rep.n_triangles == len(mesh_scene[2])


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_triangles_no_chunk_addresses(rtx, tracer, device_bvh):
    """the host builder leaves them out of the tree (order = the live triangles); the device builder takes every uploaded triangle"""
    b = ragged_chunk_scene(rtx, 16, 8)
    live = live_triangles(b[3], len(b[2]))
    assert len(live) == len(b[2]) - 3
    rep, st = build_and_audit(tracer, b, f"ragged chunks, device_bvh {device_bvh}", live=None if device_bvh else live, device_bvh=device_bvh)
    assert st["bvhBuiltOnDevice"] == device_bvh and rep.n_triangles == (len(b[2]) if device_bvh else len(live))


@pytest.fixture
def own_tracer(rtx):
    """a context of the test's own: the area-triggered rebuild counts in the context's statistics, which a neighbouring test reads"""
    with rtx.Tracer(0) as t:
        yield t


def test_local_meshes_after_upload_refit_and_the_area_triggered_rebuild(rtx, own_tracer):
    tracer = own_tracer
    mgr = rtx.scenes.mesh_test_scene(16, 8)
    mgr.numRaysPerPixel = 1
    upload_local(tracer, mgr)
    tracer.reset_accum()
    tracer.render(0, 1)
    rep0, st0 = audit_tracer(tracer, tracer.read_world_geometry()[0], "local meshes after upload")
    assert st0["bvhBuiltOnDevice"] == 1
    h = rtx.host
    for step, spread in enumerate((1.02, 6.0)):
        for i, mesh in enumerate(mgr.meshes[2:]):
            mesh.transform = h.Transform(position=mesh.transform.position * np.float32([spread, 1.0, spread]) + np.float32([0, 0.05 * i, 0]),
                                         rotation=mesh.transform.rotation, lossyScale=mesh.transform.lossyScale)
        tracer.set_mesh_transforms(mgr.build_transforms())
        tracer.render(1 + step, 1)
        st = tracer.stats()
        world = tracer.read_world_geometry()[0]
        if step == 0:                                           # a small move: the topology stays, every box is refitted
            assert st["bvhRebuilds"] == st0["bvhRebuilds"] and st["numBvhNodes"] == st0["numBvhNodes"]
            rep, _ = audit_tracer(tracer, world, "local meshes after a refit", refitted=True)
            assert rep.stack_need == rep0.stack_need
        else:                                                   # the spread trips rebuild_percent
            assert st["bvhRebuilds"] == st0["bvhRebuilds"] + 1, st["refitAreaRatio"]
            audit_tracer(tracer, world, "local meshes after the area-triggered rebuild")


@pytest.mark.parametrize("seed", [0, 3])
def test_local_meshes_in_random_poses(rtx, own_tracer, seed):
    """zero (seed 0) and negative scales, translations to 1e3 (seed 3); the second pose goes through the refit"""
    tracer = own_tracer
    rng = np.random.default_rng(500 + seed)
    mgr = rtx.scenes.mesh_test_scene(16, 8)
    mgr.numRaysPerPixel = 1
    random_pose(rtx, mgr, rng, seed)
    upload_local(tracer, mgr)
    tracer.reset_accum()
    tracer.render(0, 1)
    _, st0 = audit_tracer(tracer, tracer.read_world_geometry()[0], f"seed {seed}: first pose")
    random_pose(rtx, mgr, rng, seed)
    tracer.set_mesh_transforms(mgr.build_transforms())
    tracer.render(1, 1)
    st = tracer.stats()
    refit = st["bvhRebuilds"] == st0["bvhRebuilds"]            # (a pose that inflates the tree past rebuild_percent is rebuilt instead)
    assert not refit or st["numBvhNodes"] == st0["numBvhNodes"]
    audit_tracer(tracer, tracer.read_world_geometry()[0], f"seed {seed}: second pose ({'refit' if refit else 'rebuild'})", refitted=refit)


def test_repadding_for_a_camera_that_drifts_away(rtx, tracer):
    m = rtx.scenes.mesh_test_scene(16, 8)
    m.numRaysPerPixel, m.maxBounceCount = 1, 2
    params, spheres, tris, infos = m.build_buffers()
    extent = float(np.abs(np.concatenate([tris["posA"], tris["posB"], tris["posC"]])).max())
    tracer.set_option("kernel", 1)
    tracer.set_rows(0, int(params["height"]))
    tracer.upload(spheres=spheres[:0], triangles=tris, meshinfo=infos)
    dist, builds0 = 1.5 * extent, None
    for step in range(7):                                      # 1.5x ... 7.2x the extent: a few doublings of the padding's magnitude
        p = params.copy()
        pos = np.float32([0.3, 1.0 + 0.1 * step, -dist])
        p["worldSpaceCameraPos"] = pos
        mtx = p["camLocalToWorld"].copy(); mtx[3], mtx[7], mtx[11] = pos; p["camLocalToWorld"] = mtx
        tracer.set_params(p)
        tracer.reset_accum()
        tracer.render_frame(step)
        st = tracer.stats()
        if builds0 is None:
            builds0, repads0 = st["bvhBuilds"], st["bvhRepads"]
        assert not np.isnan(tracer.read_last_frame()).any() and st["bvhBuilds"] == builds0
        audit_tracer(tracer, tris, f"camera at {dist / extent:.2f}x the extent", refitted=st["bvhRepads"] > repads0)
        dist *= 1.3
    assert st["bvhRepads"] - repads0 >= 1


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_repadding_for_far_query_origins(rtx, shim, device_bvh):
    """origins 1e5 away widen the padding to that magnitude; an origin at 3e38 takes it to FLT_MAX (boxes of +-7e32 in f32, infinite
    in f16): every box still holds its triangles, the empty slots stay empty, the answers hold no NaN"""
    t, params, s, tr, mi = loaded_tracer(rtx, rtx.scenes.mesh_test_scene(16, 8), 0, device_bvh=device_bvh)
    with t:
        centre = np.asarray(tr["posA"]).reshape(-1, 3).mean(0).astype(np.float32)
        near = t.trace_rays(make_rays(rtx, centre[None] + np.float32([0, 9, 0]), np.float32([[0, -1, 0]])))
        assert near["kind"][0] != 0
        audit_tracer(t, tr, "before the far queries")
        repads = t.stats()["bvhRepads"]
        for far, what in ((1e5, "a query from 1e5 away"), (3e38, "a query origin of 3e38")):
            o = centre[None] + np.float32([[0, far, 0], [far, 0, 0]])
            rays = make_rays(rtx, o, centre[None] - o)
            hits = check_queries(rtx, shim, t, s, tr, mi, 0, rays, what) if far < 1e30 else t.trace_rays(rays)
            assert not np.isnan(hits["dst"]).any() and len(t.occluded(rays)) == len(rays)
            st = t.stats()
            assert st["bvhRepads"] >= repads + 1, what
            repads = st["bvhRepads"]
            audit_tracer(t, tr, what, refitted=True)
            again = t.trace_rays(make_rays(rtx, centre[None] + np.float32([0, 9, 0]), np.float32([[0, -1, 0]])))
            assert again.tobytes() == near.tobytes(), what           # the wider boxes change no answer


def test_world_space_scene_uploaded_again_and_again(rtx):
    """device_bvh = -1: host build, then two automatic device rebuilds of the moved scene, then — left alone for 20 frames — a host
    build again (test_world_space_scene_that_keeps_changing_is_rebuilt_on_the_device compares the images)"""
    m = rtx.scenes.mesh_test_scene(16, 8)
    m.numRaysPerPixel = 1
    params, spheres, tris, infos = m.build_buffers()
    with rtx.Tracer(0) as tr:
        tr.set_params(params); tr.set_rows(0, int(params["height"]))
        built = []
        for step, frames in enumerate((2, 2, 20, 2)):
            moved = tris.copy()
            for k in ("posA", "posB", "posC"):
                moved[k] = tris[k] + np.float32([0.0, 0.01 * step, 0.0])
            mi = infos.copy(); mi["boundsMin"] = infos["boundsMin"] + np.float32([0, 0.01 * step, 0]); mi["boundsMax"] = infos["boundsMax"] + np.float32([0, 0.01 * step, 0])
            tr.upload(spheres=spheres, triangles=moved, meshinfo=mi)
            tr.reset_accum()
            tr.render(0, frames)
            _, st = audit_tracer(tr, moved, f"upload {step}")
            built.append(int(st["bvhBuiltOnDevice"]))
        assert built == [0, 1, 1, 0], built


def test_one_large_device_built_tree(rtx, tracer):
    m = rtx.scenes.config3(16, 9)
    m.numRaysPerPixel = 1
    b = m.build_buffers()
    assert len(b[2]) == 100440
    rep, st = build_and_audit(tracer, b, "100,440 triangles, device builder", device_bvh=1)
    assert st["bvhBuiltOnDevice"] == 1 and rep.n_triangles == 100440


# ---- rays aimed at the box faces ---------------------------------------------------------------------------------------------------

def check_aimed(rtx, shim, t, spheres, tris, infos, what, mesh_of_chunk=None):
    rays, target = aimed_rays(rtx, tris)
    hits = check_queries(rtx, shim, t, spheres, tris, infos, 0, rays, what, mesh_of_chunk)         # == the oracle's, bit for bit
    share, unreported = aimed_ray_shares(rtx, hits, target, tris)
    assert share >= 0.90 and len(unreported) == 0, (what, share, unreported)


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_aimed_rays_through_a_built_tree(rtx, shim, device_bvh):
    t, params, s, tr, mi = loaded_tracer(rtx, rtx.scenes.mesh_test_scene(16, 8), 0, device_bvh=device_bvh)
    with t:
        check_aimed(rtx, shim, t, s, tr, mi, f"aimed rays, device_bvh {device_bvh}")
        assert t.stats()["bvhBuiltOnDevice"] == device_bvh
        audit_tracer(t, tr, f"aimed rays, device_bvh {device_bvh}")


def test_aimed_rays_through_a_refitted_tree(rtx, shim):
    mgr = rtx.scenes.mesh_test_scene(16, 8)
    params, spheres, _, _ = mgr.build_buffers()
    ltris, chunks = mgr.build_local_buffers()
    xf = mgr.build_transforms()
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres)
        t.upload_local_meshes(ltris, chunks, len(mgr.meshes))
        t.set_mesh_transforms(xf)
        t.render(0, 1)                                   # built and traced once: the next pose takes the geometry pass
        st0 = t.stats()
        xf2 = xf.copy()
        xf2["position"] += np.float32(0.75)
        xf2["rotation"][:, 1] = np.float32(0.2)
        xf2["rotation"][:, 3] = np.float32(np.sqrt(1 - 0.04))
        t.set_mesh_transforms(xf2)
        world, infos = t.read_world_geometry()
        check_aimed(rtx, shim, t, spheres, world, infos, "aimed rays, refitted pose", chunks["meshIndex"].astype(np.int32))
        st = t.stats()
        assert st["bvhRebuilds"] == st0["bvhRebuilds"] and st["numBvhNodes"] == st0["numBvhNodes"]
        audit_tracer(t, world, "aimed rays, refitted pose", refitted=True)
