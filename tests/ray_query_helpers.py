"""What the ray-query tests share: the oracle's CalculateRayCollision for caller-supplied rays (tests/ray_query_oracle.c compiled with the
CFLAGS of oracle/Makefile), the ray sets, and the scenes.  Test infrastructure only."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
SCENES = ["Balls_Outdoors", "Chess", "Knight", "Reflective_Balls", "Suzanne", "Thumbnail"]


_lib = None


def load_shim(directory=None):
    """tests/ray_query_oracle.c compiled with the CFLAGS of oracle/Makefile (once per process; into `directory`, or a temporary one)"""
    global _lib
    if _lib is None:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        cflags = re.search(r"^CFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()
        so = os.path.join(directory or tempfile.mkdtemp(prefix="ray_query_oracle_"), "librq.so")
        subprocess.check_call(["gcc", *cflags, "-shared", "-o", so, os.path.join(HERE, "ray_query_oracle.c"), "-lm"])
        lib = ctypes.CDLL(so)
        scene = [ctypes.c_void_p, ctypes.c_int] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        lib.rq_trace.argtypes = scene + [ctypes.c_int, ctypes.c_void_p]
        lib.rq_candidates.argtypes = scene + [ctypes.c_void_p]
        lib.rq_trace.restype = lib.rq_candidates.restype = ctypes.c_int
        _lib = lib
    return _lib


@pytest.fixture(scope="session")
def shim(tmp_path_factory):
    """tests/ray_query_oracle.c compiled with the CFLAGS of oracle/Makefile"""
    return load_shim(str(tmp_path_factory.mktemp("rq")))


def _buffers(rtx, spheres, tris, infos, rays):
    return (np.ascontiguousarray(spheres, rtx.SPHERE), np.ascontiguousarray(tris, rtx.TRIANGLE), np.ascontiguousarray(infos, rtx.MESHINFO),
            np.ascontiguousarray(rays, rtx.RAY).reshape(-1))


def oracle_hits(rtx, shim, spheres, tris, infos, mode, rays, accel=False):
    """HIT (n,): the closest hit of every ray on the CPU oracle, by its literal loop or (accel) its search tree"""
    s, t, m, r = _buffers(rtx, spheres, tris, infos, rays)
    out = np.zeros(len(r), rtx.HIT)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert shim.rq_trace(p(s), len(s), p(t), len(t), p(m), len(m), int(mode), p(r), len(r), 1 if accel else 0, p(out)) == 0
    return out


def oracle_candidates(rtx, shim, spheres, tris, infos, mode, rays):
    """int32 (n,): the candidates at the bit-identical dst of every ray's closest hit, the winner included (0: a miss)"""
    s, t, m, r = _buffers(rtx, spheres, tris, infos, rays)
    out = np.zeros(len(r), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert shim.rq_candidates(p(s), len(s), p(t), len(t), p(m), len(m), int(mode), p(r), len(r), p(out)) == 0
    return out


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
