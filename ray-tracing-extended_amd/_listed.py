"""What nearest.py, overlap.py and capsule.py share: one call of the closest-point entries with the listed-query options set, and the
count read from its records."""
import numpy as np

from . import _cabi

K_MAX = _cabi.HITS_MAX


def query(tracer, k, count_all, shape, pack, *args):
    """tracer.closest_points(pack(*args)) with the option `shape` (None: a point query) = 1, "closest_k" = k and "closest_all" =
    count_all -> CLOSEST records (n, k).  `pack` makes the inputs as the entry takes them once tracer and k have passed, and refuses bad
    ones (ValueError) before any C call.  The options are put back to their defaults, not to what they were."""
    if not isinstance(tracer, (_cabi.Tracer, _cabi.MultiTracer)):
        raise TypeError(f"tracer: a Tracer or a MultiTracer, not {type(tracer).__name__}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= K_MAX:
        raise ValueError(f"k: an int in 1..{K_MAX}, not {k!r}")
    inputs = pack(*args)
    # each option is put back on its own: one restoring call that raises does not keep the others from being made
    try:
        try:
            try:
                if shape:
                    tracer.set_option(shape, 1)
                tracer.set_option("closest_k", int(k))
                tracer.set_option("closest_all", 1 if count_all else 0)
                out = tracer.closest_points(inputs)
            finally:
                if shape:
                    tracer.set_option(shape, 0)
        finally:
            tracer.set_option("closest_k", 1)
    finally:
        tracer.set_option("closest_all", 0)
    # (k = 1: closest_points answers (n,) / (n, 16); the helpers' shape does not depend on k)
    return out.reshape(out.shape[0], 1, 16) if _cabi._is_tensor(out) and k == 1 else out.reshape(-1, 1) if k == 1 else out


def counts(out):
    """_reserved[0] of every input's first record -> int32 (n,), an array or a tensor as `out` is"""
    if _cabi._is_tensor(out):
        import torch
        return out[:, 0, 14].contiguous().view(torch.int32)
    return out["_reserved"][:, 0, 0].astype(np.int32)
