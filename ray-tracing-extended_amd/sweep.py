"""Sphere casts (include/rt.h "sphere casts"): how far a ball of radius r travels along each ray before it touches the scene, and where
it touches — Unity's Physics.SphereCast / CheckSphere-along-a-path, through the existing ray-query entries with option "sweep" = 1.

    sphere_cast(tracer, rays, radius)    -> HIT records (dst = the travel, hitPoint = the contact, normal = the contact normal,
                                            _reserved[0] = the contact feature: 0 sphere, 1 / 2 front / back face, 3..5 edge AB / AC / BC,
                                            6..8 vertex A / B / C)
    sphere_check(tracer, rays, radius)   -> uint8, 1 where sphere_cast would hit
    sphere_cast_all(tracer, rays, radius, max_hits=4, count_all=False)
                                         -> MULTIHIT records (n, max_hits): every primitive the ball touches, in order (Unity's
                                            Physics.SphereCastAll), through rt_trace_hits with option "hits_sweep" = 1

All take a Tracer or a MultiTracer and rays as trace_rays takes them (a RAY array, float32 (n, 8), or — a Tracer — a float32 (n, 8) CUDA
tensor, answered by the device entry with a tensor).  radius: one value for all rays or one per ray.  The radii travel as the bits of
rt_ray._reserved in a COPY of the rays; the option is set for the one call and put back to 0 in a `finally` — to 0, not to what it was:
a caller who has set "sweep" = 1 on the tracer themselves finds it cleared after either helper."""
import numpy as np

from . import _cabi


def _with_radius(rays, radius):
    """a copy of `rays` with the radii's float32 bits in the reserved word; refuses bad shapes (ValueError) before any C call"""
    if _cabi._is_tensor(rays):
        import torch
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError(f"rays: a float32 (n, 8) tensor, not {rays.dtype} {tuple(rays.shape)}")
        n = int(rays.shape[0])
        r = radius if _cabi._is_tensor(radius) else torch.as_tensor(np.asarray(radius, np.float32), device=rays.device)
        if r.dim() > 1 or (r.dim() == 1 and int(r.shape[0]) != n):
            raise ValueError(f"radius: a scalar or one value per ray ({n}), not {tuple(r.shape)}")
        out = rays.clone()
        out[:, 7] = r.to(device=rays.device, dtype=torch.float32)
        return out
    out = _cabi._ray_array(rays).copy()
    r = np.asarray(radius, np.float32)
    if r.ndim > 1 or (r.ndim == 1 and r.shape[0] != out.shape[0]):
        raise ValueError(f"radius: a scalar or one value per ray ({out.shape[0]}), not {r.shape}")
    out["_reserved"] = np.broadcast_to(r, out.shape).copy().view(np.int32)
    return out


def _swept(tracer, option, method, rays, radius, *args):
    """tracer.method(rays with the radii, *args) with `option` = 1 for that one call, put back to 0 in a `finally`"""
    if not isinstance(tracer, (_cabi.Tracer, _cabi.MultiTracer)):
        raise TypeError(f"tracer: a Tracer or a MultiTracer, not {type(tracer).__name__}")
    rays = _with_radius(rays, radius)
    tracer.set_option(option, 1)
    try:
        return getattr(tracer, method)(rays, *args)
    finally:
        tracer.set_option(option, 0)


def sphere_cast(tracer, rays, radius):
    """rt_trace_rays with option "sweep" = 1: the first contact of a ball of `radius` swept along each ray -> HIT records"""
    return _swept(tracer, "sweep", "trace_rays", rays, radius)


def sphere_check(tracer, rays, radius):
    """rt_occluded with option "sweep" = 1: 1 where a ball of `radius` swept along the ray touches something before tMax -> uint8"""
    return _swept(tracer, "sweep", "occluded", rays, radius)


def sphere_cast_all(tracer, rays, radius, max_hits=4, count_all=False):
    """rt_trace_hits with option "hits_sweep" = 1 (include/rt.h "sphere-cast-all"): the first max_hits (1..8) primitives a ball of
    `radius` touches along each ray, in order of (travel, kind, uploaded index) -> MULTIHIT records (n, max_hits).  A record's fields are
    sphere_cast's for that contact; side = which side of the face the ball's centre is on (+1 for a sphere), _reserved = the contact
    feature; count_all: hitCount counts every primitive touched before tMax.  A Tracer or a MultiTracer; rays and radius as for
    sphere_cast (a Tracer answers a CUDA tensor through the device entry, with a float32 (n, max_hits, 16) tensor).  The option is set
    for the one call and put back to 0 in a `finally`, as "sweep" is."""
    if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)) or not 1 <= max_hits <= _cabi.HITS_MAX:
        raise ValueError(f"max_hits: an integer in 1..{_cabi.HITS_MAX}, not {max_hits!r}")
    return _swept(tracer, "hits_sweep", "trace_hits", rays, radius, int(max_hits), False, bool(count_all))
