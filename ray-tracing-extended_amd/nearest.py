"""K-nearest point queries (include/rt.h "K-nearest queries"): every surface within a radius of a point, nearest first, and how many
there are — Unity's Physics.OverlapSphere, through the existing closest-point entries with the options "closest_k" and "closest_all".

    nearest_k(tracer, points, k=4, radius=None, count_all=False)  -> CLOSEST records (n, k): the k nearest candidates of every point in
                                            ascending (key, kind, uploaded index), the rest miss records; _reserved[0] of all k records =
                                            the count: min(total, k), or with count_all every candidate within the radius
    overlap_count(tracer, points, radius)   -> int32 (n,): how many spheres and triangles lie within `radius` of each point (k = 1 with
                                            count_all: the search is bounded by the radius alone)

Both take a Tracer or a MultiTracer and points as closest_points takes them (a RAY array, float32 (n, 8), or — a Tracer — a float32
(n, 8) CUDA tensor, answered by the device entry with a tensor (n, k, 16); overlap_count then returns an int32 tensor).  radius: None
keeps the radii in the points' tMax; else one value for all points or one per point, written into a COPY of the points.  The options are
set for the one call and put back to their defaults (1 and 0) in a `finally` — to the defaults, not to what they were: a caller who has
set them on the tracer themselves finds them cleared after either helper."""
import numpy as np

from . import _cabi, _listed

K_MAX = _cabi.HITS_MAX


def _with_radius(points, radius):
    """`points` as the entry takes them, with `radius` (if not None) in tMax of a copy; refuses bad shapes (ValueError) before any C call"""
    if _cabi._is_tensor(points):
        import torch
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 8:
            raise ValueError(f"points: a float32 (n, 8) tensor, not {points.dtype} {tuple(points.shape)}")
        if radius is None:
            return points
        n = int(points.shape[0])
        r = radius if _cabi._is_tensor(radius) else torch.as_tensor(np.asarray(radius, np.float32), device=points.device)
        if r.dim() > 1 or (r.dim() == 1 and int(r.shape[0]) != n):
            raise ValueError(f"radius: a scalar or one value per point ({n}), not {tuple(r.shape)}")
        out = points.clone()
        out[:, 3] = r.to(device=points.device, dtype=torch.float32)
        return out
    out = _cabi._ray_array(points)
    if radius is None:
        return out
    r = np.asarray(radius, np.float32)
    if r.ndim > 1 or (r.ndim == 1 and r.shape[0] != out.shape[0]):
        raise ValueError(f"radius: a scalar or one value per point ({out.shape[0]}), not {r.shape}")
    out = out.copy()
    out["tMax"] = r
    return out


def nearest_k(tracer, points, k=4, radius=None, count_all=False):
    """rt_closest_points with option "closest_k" = k (and "closest_all" = count_all): the k nearest surfaces of every point -> CLOSEST
    records (n, k)"""
    return _listed.query(tracer, k, count_all, None, _with_radius, points, radius)


def overlap_count(tracer, points, radius):
    """Physics.OverlapSphere's count: the number of spheres and triangles with key < radius * radius, per point -> int32 (n,)"""
    return _listed.counts(_listed.query(tracer, 1, True, None, _with_radius, points, radius))
