"""What the checkers of the listed point queries share — K-nearest (nearest_check.py), box overlap (overlap_check.py) and capsule overlap
(capsule_check.py), whose C entries np_nearest, ov_overlap and cp_capsule have one signature: the ctypes binding of that signature and
the one call through it, the word-for-word comparison of (n, K) records, the count word, and the bounds of a scene for the batches.
Each family's module keeps its variants, forms, batch and twins.  Test infrastructure only."""
import ctypes

import numpy as np

import closest_check as cc


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def bind_listed(fn):
    """the signature of np_nearest / ov_overlap / cp_capsule: spheres, ns, triangles, nt, meshinfo, nm, chunk_mesh, inputs, n, K, all,
    variant, out, totals, kth_ties"""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    fn.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp]
    fn.restype = ci
    return fn


def oracle_listed(lib_fn, rtx, spheres, tris, infos, inputs, k, count_all=0, chunk_mesh=None, variant=0, totals=None, kth_ties=None):
    """CLOSEST (n, k): the brute-force answer of `lib_fn` (bound by bind_listed) for every input.  totals / kth_ties: int32 (n,) arrays that
    receive, per input, the number of all candidates that count and whether the k-th and (k+1)-th keys of the full sort are bit-equal"""
    s = np.ascontiguousarray(spheres, rtx.SPHERE)
    t = np.ascontiguousarray(tris, rtx.TRIANGLE)
    m = np.ascontiguousarray(infos, rtx.MESHINFO)
    r = np.ascontiguousarray(inputs, rtx.RAY).reshape(-1)
    cm = None if chunk_mesh is None else np.ascontiguousarray(chunk_mesh, np.int32)
    assert cm is None or len(cm) == len(m)
    for a in (totals, kth_ties):
        assert a is None or (a.dtype == np.int32 and a.shape == (len(r),) and a.flags.c_contiguous)
    out = np.zeros((len(r), int(k)), rtx.CLOSEST)
    rc = lib_fn(_p(s), len(s), _p(t), len(t), _p(m), len(m), _p(cm), _p(r), len(r), int(k), int(count_all), int(variant),
                _p(out), _p(totals), _p(kth_ties))
    assert rc == 0, f"{lib_fn.__name__} failed: {rc}"
    return out


def words(rtx, records):
    """the records as uint32 (..., 16)"""
    a = np.ascontiguousarray(records, rtx.CLOSEST)
    return a.view(np.uint32).reshape(a.shape + (16,))


COUNT_WORD = 14                                      # _reserved[0] among a record's 16 words


def counts(records):
    return records["_reserved"][..., 0]


def assert_same_records(rtx, got, want, what):
    """every word of every record (closest_check's comparison) and the shape (n, K)"""
    got, want = np.ascontiguousarray(got, rtx.CLOSEST), np.ascontiguousarray(want, rtx.CLOSEST)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    cc.assert_same_records(rtx, got, want, what)


def assert_first_is_the_default(rtx, got, default, what):
    """record 0 of any form equals the default call's record in every word but _reserved[0]"""
    g, d = words(rtx, np.ascontiguousarray(got, rtx.CLOSEST)[:, 0]).copy(), words(rtx, default).copy()
    assert (d[:, COUNT_WORD:] == 0).all(), what
    g[:, COUNT_WORD] = 0
    cc.assert_same_records(rtx, g.view(rtx.CLOSEST).reshape(-1), d.view(rtx.CLOSEST).reshape(-1), what + ": record 0 against the default call")


def different(rtx, a, b):
    return not np.array_equal(words(rtx, a), words(rtx, b))


def _live(m):
    """the uploaded indices of the triangles the chunks address, chunk by chunk"""
    return np.concatenate([np.arange(i["firstTriangleIndex"], i["firstTriangleIndex"] + i["numTriangles"]) for i in m]) if len(m) else np.zeros(0, int)


def scene_bounds(s, t, m):
    """(lo, hi) float64 over every addressed triangle corner and every sphere's box"""
    live = _live(m)
    parts = [np.asarray(t[k][live], np.float64).reshape(-1, 3) for k in ("posA", "posB", "posC")] if len(live) else []
    if len(s):
        c, r = np.asarray(s["position"], np.float64), np.asarray(s["radius"], np.float64)[:, None]
        parts += [c - r, c + r]
    allp = np.concatenate(parts)
    return allp.min(0), allp.max(0)
