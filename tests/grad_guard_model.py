"""The gradient guard's definition (include/nerf_amd.h) in numpy, for the tests to hold the kernels to:

    S    = sum g_i^2 in float64 (a square of an fp32 value is exact there; math.fsum adds them without error)
    norm = fl32(sqrt(S))
    skip <=> norm is not finite
    coef = min(1, max_norm / (norm + 1e-6)): three fp32 operations, each rounded on its own (torch's clip_grad_norm_)
"""
import math

import numpy as np

F32 = np.float32


def norm64(g):
    """sqrt(sum g_i^2) in float64 (NaN / inf where the gradient holds one)."""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    if not np.isfinite(g).all():
        return float("nan") if np.isnan(g).any() else float("inf")
    return math.sqrt(math.fsum(g * g))


def norm32(g):
    """The norm as the record holds it: the float64 norm rounded to fp32 (inf where it exceeds the fp32 range)."""
    with np.errstate(over="ignore"):
        return F32(norm64(g))


def skip(norm):
    return not np.isfinite(F32(norm))


def coef(max_norm, norm):
    """torch's rule on fp32 scalars; 0 on a skipped step."""
    if skip(norm):
        return F32(0)
    with np.errstate(over="ignore"):
        return np.minimum(F32(1), F32(max_norm) / (F32(norm) + F32(1e-6)))


def ulp(x):
    """The spacing of fp32 at |x|."""
    return float(np.spacing(np.abs(F32(x))))
