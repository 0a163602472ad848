"""Capsule overlap queries (include/rt.h "capsule overlap queries"): every surface within `radius` of a segment, nearest first, where on
the surface, where on the segment, and how many there are — over the closest-point entries with the option "closest_capsule" (and
"closest_k" / "closest_all" for the records and the count).

    overlap_capsule(tracer, p0, p1, radius, k=4, count_all=False)  -> CLOSEST records (n, k): the k candidates nearest to the segment
                                                                     p0 .. p1 within `radius` (Physics.OverlapCapsule)
    check_capsule(tracer, p0, p1, radius)                          -> uint8 (n,): 1 where something lies within `radius` (CheckCapsule)
    closest_to_segment(tracer, p0, p1, radius=inf)                 -> (records (n,), s float32 (n,)): the nearest surface to each segment
                                                                     and the parameter of the segment's closest point, x = p0 + (p1 - p0) s

A Tracer or a MultiTracer; p0 and p1 float32 (n, 3) and radius a scalar or (n,), as numpy arrays or — a Tracer — CUDA tensors, answered
by the device entry with a tensor (n, k, 16) / uint8 (n,) / ((n, 16), (n,)).  d = p1 - p0 is formed in float32.  The three options are set
for the one call and put back to their defaults (0, 1 and 0) in nested `finally` blocks — to the defaults, not to what they were."""
import numpy as np

from . import _cabi, _listed

K_MAX = _cabi.HITS_MAX


def _segments(p0, p1, radius):
    """the segments as the entry takes them — a RAY array, or a float32 (n, 8) tensor where p0 is a tensor: origin = p0, tMax = radius,
    direction = p1 - p0; refuses bad shapes (ValueError) before any C call"""
    if _cabi._is_tensor(p0):
        import torch
        for name, a in (("p0", p0), ("p1", p1)):
            if not _cabi._is_tensor(a) or a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
                raise ValueError(f"{name}: a float32 (n, 3) tensor like p0, not {getattr(a, 'dtype', type(a).__name__)} {tuple(getattr(a, 'shape', ()))}")
        n = int(p0.shape[0])
        if tuple(p1.shape) != (n, 3):
            raise ValueError(f"p1: ({n}, 3) like p0, not {tuple(p1.shape)}")
        r = radius if _cabi._is_tensor(radius) else torch.as_tensor(np.asarray(radius, np.float32), device=p0.device)
        if tuple(r.shape) not in ((), (n,)):
            raise ValueError(f"radius: a scalar or ({n},), not {tuple(r.shape)}")
        out = torch.zeros((n, 8), dtype=torch.float32, device=p0.device)
        out[:, 0:3] = p0
        out[:, 3] = r.to(device=p0.device, dtype=torch.float32)
        out[:, 4:7] = p1.to(p0.device) - p0
        return out
    a, b = np.asarray(p0), np.asarray(p1)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "fiu":
        raise ValueError(f"p0: a float32 (n, 3) array, not {a.dtype} {a.shape}")
    if b.shape != a.shape or b.dtype.kind not in "fiu":
        raise ValueError(f"p1: {a.shape} like p0, not {b.dtype} {b.shape}")
    r = np.asarray(radius)
    if r.dtype.kind not in "fiu" or r.shape not in ((), (a.shape[0],)):
        raise ValueError(f"radius: a scalar or ({a.shape[0]},), not {r.dtype} {r.shape}")
    out = np.zeros(a.shape[0], _cabi.RAY)
    out["origin"] = a
    out["tMax"] = r
    out["direction"] = b.astype(np.float32) - a.astype(np.float32)
    return out


def overlap_capsule(tracer, p0, p1, radius, k=4, count_all=False):
    """Physics.OverlapCapsule: rt_closest_points with "closest_capsule" = 1 and "closest_k" = k (and "closest_all" = count_all) -> CLOSEST
    records (n, k); _reserved[1] of a record holds the bits of s"""
    return _listed.query(tracer, k, count_all, "closest_capsule", _segments, p0, p1, radius)


def check_capsule(tracer, p0, p1, radius):
    """Physics.CheckCapsule: 1 where a sphere or a triangle lies within `radius` of the segment -> uint8 (n,)"""
    c = _listed.counts(_listed.query(tracer, 1, False, "closest_capsule", _segments, p0, p1, radius))
    if _cabi._is_tensor(c):
        import torch
        return (c != 0).to(torch.uint8)
    return (c != 0).astype(np.uint8)


def closest_to_segment(tracer, p0, p1, radius=np.inf):
    """the nearest surface to each segment -> (records (n,), s float32 (n,)), s read from _reserved[1]: x = p0 + (p1 - p0) * s"""
    out = _listed.query(tracer, 1, False, "closest_capsule", _segments, p0, p1, radius)
    if _cabi._is_tensor(out):
        rec = out[:, 0, :]
        return rec, rec[:, 15].contiguous()
    rec = np.ascontiguousarray(out[:, 0])
    return rec, np.ascontiguousarray(rec["_reserved"][:, 1]).view(np.float32)
