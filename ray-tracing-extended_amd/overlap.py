"""Box overlap queries (include/rt.h "box overlap queries"): every surface that touches an axis-aligned box, nearest to the box's centre
first, and how many there are — Unity's Physics.OverlapBox / CheckBox, through the existing closest-point entries with the option
"closest_box" (and "closest_k" / "closest_all" for the records and the count).

    overlap_box(tracer, centres, half_extents, k=4, count_all=False)  -> CLOSEST records (n, k): the k touching candidates nearest to
                                            each box's centre in ascending (key, kind, uploaded index), the rest miss records;
                                            _reserved[0] of all k records = the count: min(total, k), or with count_all every
                                            candidate that touches
    check_box(tracer, centres, half_extents)    -> uint8 (n,): 1 where anything touches the box (k = 1: the count is 0 or 1)
    voxel_counts(tracer, lo, hi, shape)         -> int32 array of `shape`: how many spheres and triangles touch each cell of the grid
                                            that divides [lo, hi] into shape = (nx, ny, nz) cells (conservative voxelisation: one box
                                            per cell, k = 1 with count_all), asked in chunks no longer than one slice

overlap_box and check_box take a Tracer or a MultiTracer; centres float32 (n, 3) and half_extents (n, 3), (3,) or a scalar as numpy
arrays, or — a Tracer — CUDA tensors, answered by the device entry with a tensor (n, k, 16) / uint8 (n,).  The three options are set for
the one call and put back to their defaults (0, 1 and 0) in a `finally` — to the defaults, not to what they were."""
import numpy as np

from . import _cabi, _listed

K_MAX = _cabi.HITS_MAX
CHUNK = 1 << 22                 # cells per call of voxel_counts: the largest "closest_slice" (k = 1)


def _boxes(centres, half_extents):
    """the boxes as the entry takes them — a RAY array, or a float32 (n, 8) tensor where centres is a tensor: origin = centre, tMax = 1
    (only a gate), direction = half-extents; refuses bad shapes (ValueError) before any C call"""
    if _cabi._is_tensor(centres):
        import torch
        if centres.dtype != torch.float32 or centres.dim() != 2 or centres.shape[1] != 3:
            raise ValueError(f"centres: a float32 (n, 3) tensor, not {centres.dtype} {tuple(centres.shape)}")
        n = int(centres.shape[0])
        h = half_extents if _cabi._is_tensor(half_extents) else torch.as_tensor(np.asarray(half_extents, np.float32), device=centres.device)
        if tuple(h.shape) not in ((), (3,), (n, 3)):
            raise ValueError(f"half_extents: a scalar, (3,) or ({n}, 3), not {tuple(h.shape)}")
        out = torch.zeros((n, 8), dtype=torch.float32, device=centres.device)
        out[:, 0:3] = centres
        out[:, 3] = 1.0
        out[:, 4:7] = h.to(device=centres.device, dtype=torch.float32)
        return out
    c = np.asarray(centres)
    if c.ndim != 2 or c.shape[1] != 3 or c.dtype.kind not in "fiu":
        raise ValueError(f"centres: a float32 (n, 3) array, not {c.dtype} {c.shape}")
    h = np.asarray(half_extents)
    if h.dtype.kind not in "fiu" or h.shape not in ((), (3,), (c.shape[0], 3)):
        raise ValueError(f"half_extents: a scalar, (3,) or ({c.shape[0]}, 3), not {h.dtype} {h.shape}")
    out = np.zeros(c.shape[0], _cabi.RAY)
    out["origin"] = c
    out["tMax"] = 1.0
    out["direction"] = h
    return out


def overlap_box(tracer, centres, half_extents, k=4, count_all=False):
    """Physics.OverlapBox: rt_closest_points with "closest_box" = 1 and "closest_k" = k (and "closest_all" = count_all) -> CLOSEST
    records (n, k)"""
    return _listed.query(tracer, k, count_all, "closest_box", _boxes, centres, half_extents)


def check_box(tracer, centres, half_extents):
    """Physics.CheckBox: 1 where a sphere or a triangle touches the box -> uint8 (n,)"""
    c = _listed.counts(_listed.query(tracer, 1, False, "closest_box", _boxes, centres, half_extents))
    if _cabi._is_tensor(c):
        import torch
        return (c != 0).to(torch.uint8)
    return (c != 0).astype(np.uint8)


def voxel_counts(tracer, lo, hi, shape):
    """The number of spheres and triangles that touch each cell of the (nx, ny, nz) grid over [lo, hi] -> int32 array of `shape`.  Cell
    (i, j, k) is the box of half-extents (hi - lo) / shape / 2 around lo + (index + 1/2) * (hi - lo) / shape, all in float32; neighbouring
    cells share their faces up to that rounding, and a surface on a shared face counts in both (touching counts)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    dims = tuple(int(d) for d in np.atleast_1d(np.asarray(shape)))
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError(f"lo, hi: two finite (3,) corners with hi >= lo, not {lo!r}, {hi!r}")
    if len(dims) != 3 or min(dims) < 1 or np.asarray(shape).dtype.kind not in "iu":
        raise ValueError(f"shape: three positive ints, not {shape!r}")
    cell = (hi - lo) / np.float32(dims)
    half = cell * np.float32(0.5)
    n = dims[0] * dims[1] * dims[2]
    out = np.empty(n, np.int32)
    for first in range(0, n, CHUNK):
        idx = np.arange(first, min(first + CHUNK, n))
        ijk = np.stack(np.unravel_index(idx, dims), 1).astype(np.float32)
        centres = lo + (ijk + np.float32(0.5)) * cell
        out[idx] = _listed.counts(_listed.query(tracer, 1, True, "closest_box", _boxes, centres.astype(np.float32), half))
    return out.reshape(dims)
