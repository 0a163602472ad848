"""The checker of sphere-cast-all: tests/sweep_all_oracle.c bound with ctypes.  The batch the GPU tests and the CPU tests share is the
sphere casts' own, sweep_check.batch_of's 710 rays, with nothing added: tests/test_sweep_all_cpu.py asserts that on `mixed` and `Knight`
it fills, overflows and ties the list often enough.  Test infrastructure only."""
import ctypes

import numpy as np

import hits_check as hc
import sweep_check as sc
from checker_build import compile_checker

KS = (1, 2, 3, 8)
SHARED_WORDS = 13               # words 0..12 of a record, dst .. v: what rt_multihit shares with the sphere cast's rt_hit

_lib = None


def lib(directory=None):
    global _lib
    if _lib is None:
        so = compile_checker("sweep_all_oracle.c", directory)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        so.swa_cast.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, ci, ci, ci, vp]
        so.swa_cast.restype = ci
        _lib = so
    return _lib


def oracle_cast_all(rtx, spheres, tris, infos, rays, K=4, count_all=False, chunk_mesh=None):
    """MULTIHIT (n, K): the brute-force list of every ray"""
    s = np.ascontiguousarray(spheres, rtx.SPHERE)
    t = np.ascontiguousarray(tris, rtx.TRIANGLE)
    m = np.ascontiguousarray(infos, rtx.MESHINFO)
    r = np.ascontiguousarray(rays, rtx.RAY).reshape(-1)
    cm = None if chunk_mesh is None else np.ascontiguousarray(chunk_mesh, np.int32)
    assert cm is None or len(cm) == len(m)
    out = np.zeros((len(r), K), rtx.MULTIHIT)
    p = sc._p
    rc = lib().swa_cast(p(s), len(s), p(t), len(t), p(m), len(m), p(cm), p(r), len(r), int(K), int(bool(count_all)), p(out))
    assert rc == 0, f"swa_cast failed: {rc}"
    return out


assert_same_records = hc.assert_same_records


def words(records):
    """uint32 (..., 16): the records as words"""
    a = np.ascontiguousarray(records)
    return a.view(np.uint32).reshape(a.shape + (16,))
