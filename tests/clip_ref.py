"""Float64 numpy restatement of gradient clipping (sr_amd.grad_clip, csrc/grad_clip.hip), independent of the package:
torch.nn.utils.clip_grad_norm_ with norm_type 2 and clip_grad_value_.

    total_norm = sqrt(sum over every array of sum(g^2))           coef = min(1, max_norm / (total_norm + 1e-6))
    clip_by_norm : g * coef                                       clip_by_value : g < -b ? -b : (g > b ? b : g)   (a NaN stays a NaN)

tests/test_grad_clip_cpu.py pins these against the torch functions on float64 tensors."""
import math

import numpy as np


def total_norm(arrays, scale=1.0):
    """The 2-norm of all `arrays` together, summed in float64, divided by `scale` (the loss scale the arrays still carry)."""
    return math.sqrt(sum(float(np.sum(np.square(np.asarray(a, dtype=np.float64)))) for a in arrays)) / float(scale)


def coef(norm, max_norm):
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def clip_by_norm(arrays, max_norm, scale=1.0):
    """(clipped float64 arrays, total norm, coefficient)."""
    n = total_norm(arrays, scale)
    c = coef(n, max_norm)
    return [np.asarray(a, dtype=np.float64) * c for a in arrays], n, c


def clip_by_value(arrays, bound):
    """Every array clamped to [-bound, bound] in its own dtype (`bound` is rounded to it); NaN elements stay NaN."""
    out = []
    for a in arrays:
        a = np.asarray(a)
        b = a.dtype.type(bound)
        out.append(np.where(a < -b, -b, np.where(a > b, b, a)).astype(a.dtype))
    return out
