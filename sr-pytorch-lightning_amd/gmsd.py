"""GMSD (Xue, Zhang, Mou, Bovik: "Gradient magnitude similarity deviation: a highly efficient perceptual image quality index",
2014) as a training loss and a validation metric: piq.GMSDLoss, called like the model's other piq losses on clamp(sr, 0, 1) and hr.
An edge-aware term that, unlike the reference's `edge_loss` (computed under no_grad), gives the model a gradient.  Part of `ops`
(re-exported there).

For a test image x = clamp(sr, 0, 1) and a reference y = hr, both N x C x H x W with C = 1 or 3 (anything else: ValueError):
  1. luma: C = 3: Y = 0.299 R + 0.587 G + 0.114 B (the first row of piq's RGB -> YIQ); C = 1: the plane itself;
  2. pooling: p = max(H % 2, W % 2) rows of zeros at the bottom and p columns of zeros at the right (piq's zero pad, kept as it is:
     with an odd size the last pooled row / column averages real pixels with zeros), then the 2 x 2 average with stride 2 and floor:
     Hd = (H + p) // 2, Wd = (W + p) // 2 (a pad row / column that the floor drops plays no part);
  3. gradient magnitude: kx = [[-1, 0, 1]] x 3 / 3, ky = kx^T as a cross-correlation with zero padding 1 (the map stays Hd x Wd),
     a = sqrt(gx^2 + gy^2) of x, b of y;
  4. GMS = (2ab + c) / (a^2 + b^2 + c), c = 170 / 255^2;
  5. GMSD_n = the population standard deviation of GMS over the Hd x Wd positions of image n;
  6. loss = metric = mean over n of GMSD_n: the value itself, 0 is a perfect match.

Both paths work with d = GMS - 1 = -(a - b)^2 / (a^2 + b^2 + c): the same deviation, no cancellation near GMS = 1, and exactly 0 for
identical images.

Gradient: with respect to sr only; the clamp passes it on the closed interval [0, 1] (torch's convention).

Departures and limits, on both paths:
  - where gx = gy = 0 the derivative of the square root is taken as 0 (piq's autograd gives NaN on every flat region, and clamped
    highlights are flat);
  - an image whose variance of GMS is exactly 0 gets a zero gradient (piq gives NaN or inf; sr identical to hr is such an image);
  - hr is not range-checked: that needs a host sync, which a captured training step cannot do;
  - parity with piq itself is not pinned (piq is not a dependency): tests/gmsd_ref.py states the definition in float64.
"""
import torch
import torch.nn.functional as F

from . import _lib as L
from .ops import _f32c, _need_gpu, _ptr, _stream      # (ops.py imports this module at its END: these exist by then)

__all__ = ["gmsd_torch", "GMSDLossFn", "gmsd_loss", "gmsd"]

C_GMS = 170.0 / 255.0 ** 2
LUMA = (0.299, 0.587, 0.114)


def _check(x, y):
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"GMSD needs two N x C x H x W images of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[1] not in (1, 3):
        raise ValueError(f"GMSD needs 1 or 3 channels, got {x.shape[1]}")
    if x.numel() == 0:
        raise ValueError(f"GMSD needs non-empty images, got {tuple(x.shape)}")


def _pooled_luma(t):
    if t.shape[1] == 3:
        t = LUMA[0] * t[:, 0:1] + LUMA[1] * t[:, 1:2] + LUMA[2] * t[:, 2:3]
    p = max(t.shape[-2] % 2, t.shape[-1] % 2)
    if p:
        t = F.pad(t, [0, p, 0, p])
    return F.avg_pool2d(t, 2)


def _prewitt(p):
    """(gx, gy) of an N x 1 x Hd x Wd plane: right minus left columns and bottom minus top rows of the zero-padded plane, over 3."""
    q = F.pad(p, [1, 1, 1, 1])
    top, mid, bot = q[..., :-2, :], q[..., 1:-1, :], q[..., 2:, :]
    gx = ((top[..., 2:] - top[..., :-2]) + (mid[..., 2:] - mid[..., :-2]) + (bot[..., 2:] - bot[..., :-2])) / 3.0
    gy = ((bot[..., :-2] - top[..., :-2]) + (bot[..., 1:-1] - top[..., 1:-1]) + (bot[..., 2:] - top[..., 2:])) / 3.0
    return gx, gy


def _sqrt0(s):
    """sqrt(s) whose derivative at s = 0 is taken as 0 (s >= 0)."""
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def gmsd_torch(x, y):
    """GMSD (mean over images, 0-d) of test image `x` against reference `y` in plain torch (fp32 or float64, any device).  No clamp:
    `gmsd_loss` clamps sr as the model does."""
    _check(x, y)
    dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    gxx, gyx = _prewitt(_pooled_luma(x.to(dt)))
    gxy, gyy = _prewitt(_pooled_luma(y.to(dt)))
    sa, sb = gxx * gxx + gyx * gyx, gxy * gxy + gyy * gyy
    d = -(_sqrt0(sa) - _sqrt0(sb)) ** 2 / (sa + sb + C_GMS)                     # GMS - 1
    var = ((d - d.mean(dim=(1, 2, 3), keepdim=True)) ** 2).mean(dim=(1, 2, 3))
    return _sqrt0(var).mean()


# --------------------------------------------------------------------------------------------
# HIP path (csrc/gmsd.hip)
# --------------------------------------------------------------------------------------------
def _args(s, h, *, partial=None, stats=None, loss=None, gout=None, grad=None):
    n, c, hh, ww = s.shape
    return L.GmsdArgs(sr=s.data_ptr(), hr=h.data_ptr(), N=n, C=c, H=hh, W=ww, partial=_ptr(partial), stats=_ptr(stats),
                      loss=_ptr(loss), gout=_ptr(gout), grad=_ptr(grad))


def _forward(s, h):
    """The two forward entry points on contiguous fp32 CUDA tensors: (loss, stats)."""
    nt = L.load().srk_gmsd_tiles(*s.shape)
    if nt <= 0:
        raise ValueError(f"GMSD: sizes {tuple(s.shape)} refused")
    partial = torch.empty(nt, 2, dtype=torch.float64, device=s.device)
    stats = torch.empty(s.shape[0], 2, dtype=torch.float32, device=s.device)
    loss = torch.empty((), dtype=torch.float32, device=s.device)
    a = _args(s, h, partial=partial, stats=stats, loss=loss)
    L.call("srk_gmsd_fwd", a, _stream())
    L.call("srk_gmsd_finalize", a, _stream())
    return loss, stats


class GMSDLossFn(torch.autograd.Function):
    """GMSD(clamp(sr, 0, 1), hr) as two entry points forward (srk_gmsd_fwd: clamp, luma, pooling, the Prewitt taps and the per-tile
    sums of GMS - 1 and its square; srk_gmsd_finalize: the fixed-order reductions, each image's mean and deviation, the loss) and
    one backward launch (srk_gmsd_bwd: recomputes each tile's maps from sr and hr on a 2-position halo, scaled by the upstream
    gradient read on the device: capturable), which writes every element of the gradient.  Nothing but sr, hr and two floats per
    image is kept for the backward."""

    @staticmethod
    def forward(ctx, sr, hr):
        _need_gpu(sr)
        _check(sr, hr)
        s, h = _f32c(sr), _f32c(hr)
        loss, stats = _forward(s, h)
        ctx.save_for_backward(s, h, stats)
        return loss

    @staticmethod
    def backward(ctx, g):
        s, h, stats = ctx.saved_tensors
        gout = g.detach().float().contiguous()
        grad = torch.empty_like(s)                 # every pixel belongs to a pooled pixel: the kernel writes all of it
        L.call("srk_gmsd_bwd", _args(s, h, stats=stats, gout=gout, grad=grad), _stream())
        return grad, None


def _hip_ok(sr, hr):
    return (sr.is_cuda and hr.is_cuda and sr.dtype == torch.float32 and hr.dtype == torch.float32 and sr.is_contiguous()
            and hr.is_contiguous())


def gmsd_loss(sr, hr):
    """GMSD(clamp(sr, 0, 1), hr): HIP for contiguous CUDA fp32 tensors when `hr` needs no gradient, `gmsd_torch` otherwise
    (a strided view goes to the torch statement, which reads it in place, rather than through a hidden copy)."""
    _check(sr, hr)
    if hr.requires_grad or not _hip_ok(sr, hr):
        return gmsd_torch(sr.clamp(0, 1), hr)
    return GMSDLossFn.apply(sr, hr)


def gmsd(x, y):
    """The metric: the loss's value, GMSD(clamp(x, 0, 1), y), without a gradient.  On contiguous CUDA fp32 tensors the forward
    launches only; `gmsd_torch` otherwise.  (The model calls it on images it has already clamped.)"""
    _check(x, y)
    with torch.no_grad():
        if _hip_ok(x, y):
            return _forward(x.detach(), y.detach())[0]
        return gmsd_torch(x.detach().clamp(0, 1), y.detach())
