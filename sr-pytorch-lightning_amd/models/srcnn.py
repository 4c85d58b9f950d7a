"""SRCNN (models/srcnn.py:9-27): BASELINE config 0, the reference's own CPU-runnable plumbing case.

NOT part of the HIP hot path: bicubic interpolation + 9x9/1x1/5x5 convs in
plain PyTorch on whatever device the tensors live on.  It exists so that the `SRModel` surface
(ctor, training_step, configure_optimizers) can be exercised without a GPU.
"""
import contextlib
from typing import Any

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .srmodel import SRModel


@contextlib.contextmanager
def _deterministic_convs():
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = prev


class _RepeatableConvFn(torch.autograd.Function):
    """torch's own convolution on a GPU, forward and backward, with its deterministic algorithms: the default weight-gradient algorithm
    there adds its partial sums with float atomics, and the gradients of one backward pass computed twice differ in their last bits
    ("Reproducibility").  The backward pass runs outside `forward`, so the switch has to be set in both places."""

    @staticmethod
    def forward(ctx, x, w, b, padding):
        ctx.save_for_backward(x, w)
        ctx.padding, ctx.has_b = padding, b is not None
        with _deterministic_convs():
            return F.conv2d(x, w, b, padding=padding)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        p = ctx.padding
        mask = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_b and ctx.needs_input_grad[2]]
        with _deterministic_convs():
            gx, gw, gb = torch.ops.aten.convolution_backward(g.contiguous(), x, w, [w.shape[0]] if ctx.has_b else None, [1, 1], [p, p], [1, 1],
                                                             False, [0, 0], 1, mask)
        return (gx if mask[0] else None), (gw if mask[1] else None), (gb if mask[2] else None), None


class SRCNN(SRModel):
    def __init__(self, **kwargs: dict[str, Any]):
        super().__init__(**kwargs)
        self._net = nn.Sequential(nn.Conv2d(self._channels, 64, 9, padding=4), nn.ReLU(True),
                                  nn.Conv2d(64, 32, 1, padding=0), nn.ReLU(True),
                                  nn.Conv2d(32, self._channels, 5, padding=2))

    def forward(self, x):
        x = F.interpolate(x, scale_factor=self._scale_factor, mode='bicubic')
        for m in self._net:
            if x.is_cuda and isinstance(m, nn.Conv2d):
                x = _RepeatableConvFn.apply(x, m.weight, m.bias, m.padding[0])
            else:
                x = m(x)
            if isinstance(m, nn.ReLU):
                x = ops.cut(x)              # segment boundary (identity unless ops.record_segments is active)
        return x
