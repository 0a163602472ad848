"""What the query tests share besides their checker (tests/query_check.py): its library as a fixture, the ray sets, and the scenes.
Test infrastructure only."""
import os

import numpy as np
import pytest

import query_check

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SCENES = ["Balls_Outdoors", "Chess", "Knight", "Reflective_Balls", "Suzanne", "Thumbnail"]


def load_shim(directory=None):
    """the query checkers' library (tests/query_oracle.c; once per process; built into `directory`, or a temporary one)"""
    return query_check.lib(directory)


@pytest.fixture(scope="session")
def shim(tmp_path_factory):
    """the query checkers' library (tests/query_oracle.c compiled with the CFLAGS of oracle/Makefile)"""
    return load_shim(str(tmp_path_factory.mktemp("rq")))


def make_rays(rtx, origins, directions, t_max=np.inf):
    r = np.zeros(len(origins), rtx.RAY)
    r["origin"], r["direction"], r["tMax"] = origins, directions, t_max
    return r


def camera_rays(rtx, params, w=64, h=48):
    """pinhole rays through pixel centres (normalised directions, as the renderer's camera rays are)"""
    M = np.asarray(params["camLocalToWorld"], np.float32).reshape(4, 4)
    vp = np.asarray(params["viewParams"], np.float32)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    lx, ly = ((xs + 0.5) / w - 0.5) * vp[0], ((ys + 0.5) / h - 0.5) * vp[1]
    local = np.stack([lx.ravel(), ly.ravel(), np.full(lx.size, vp[2], np.float32), np.ones(lx.size, np.float32)], 1)
    focus = (local @ M.T)[:, :3]
    pos = np.asarray(params["worldSpaceCameraPos"], np.float32)
    d = focus - pos
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return make_rays(rtx, np.broadcast_to(pos, d.shape), d.astype(np.float32))


def scene_of(rtx, name):
    from rtx_amd import unity_scene
    if name == "mesh_test_scene":
        return rtx.scenes.mesh_test_scene(64, 48)
    return unity_scene.load_scene_npz(os.path.join(GOLDEN, "scenes", name + ".npz"), 64, 48)


def random_rays(rtx, tris, spheres, n, seed):
    rng = np.random.default_rng(seed)
    pts = [np.asarray(tris["posA"]).reshape(-1, 3), np.asarray(spheres["position"]).reshape(-1, 3)]
    pts = np.concatenate([p for p in pts if len(p)]) if any(len(p) for p in pts) else np.zeros((1, 3), np.float32)
    lo, hi = pts.min(0), pts.max(0)
    ext = np.maximum(hi - lo, 1.0)
    o = (lo - ext + rng.random((n, 3)) * 3 * ext).astype(np.float32)          # inside and outside the bounds
    d = rng.standard_normal((n, 3)).astype(np.float32)                         # not normalised
    k = n // 8                                                                 # axis-aligned, zero components
    d[:k] = 0.0
    d[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0, 2.5], k)
    d[k:2 * k, rng.integers(0, 3)] = 0.0
    return make_rays(rtx, o, d)
