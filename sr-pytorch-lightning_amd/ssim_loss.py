"""SSIM (Wang, Bovik, Sheikh, Simoncelli: "Image quality assessment: from error visibility to structural similarity", 2004) as a
training loss, 1 - SSIM with piq.ssim's defaults (piq.SSIMLoss; the structural term of Zhao et al.'s "0.16*l1+0.84*ssim"), called
like the model's other piq losses on clamp(sr, 0, 1) and hr.  Part of `ops` (re-exported there).

For a test image x = clamp(sr, 0, 1) and a reference y = hr, both N x C x H x W with any C >= 1:
  1. f = max(1, round(min(H, W) / 256)) (Python's round); f > 1: both images are avg_pool2d(f), remainder rows / columns dropped
     (Hp = H // f, Wp = W // f); Hp, Wp >= 11;
  2. G: the separable 11-tap Gaussian, sigma 1.5, normalised; over the valid (Hp - 10) x (Wp - 10) positions
     mu_x = G*x, mu_y = G*y, s_xx = G*x^2 - mu_x^2, s_yy = G*y^2 - mu_y^2, s_xy = G*xy - mu_x mu_y, c1 = 1e-4, c2 = 9e-4,
     S = (2 mu_x mu_y + c1)(2 s_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(s_xx + s_yy + c2));
  3. loss = 1 - mean over images of (mean over channels of (mean of S)): on in-range input 1 - srmodel._ssim(x, y).

Gradient: with respect to sr only; the clamp passes it on the closed interval [0, 1] (torch's convention), the dropped remainder
rows / columns get 0.

Departures and limits, on both paths:
  - piq asserts 0 <= y <= 1; that check needs a host sync, which a captured training step cannot do, so hr is not checked;
  - parity with piq itself is not pinned (piq is not a dependency): tests/ssim_loss_ref.py states the definition in float64.
"""
import torch
import torch.nn.functional as F

from . import _lib as L
from .ops import _f32c, _need_gpu, _ptr, _stream      # (ops.py imports this module at its END: these exist by then)

__all__ = ["ssim_torch", "SSIMLossFn", "ssim_loss"]

KERNEL_SIZE, SIGMA, C1, C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2
# Both paths filter x - 1/2 and y - 1/2 and give the means the 1/2 back: the (co)variances do not see a shift, and in fp32
# G*x'^2 - (G*x')^2 then loses several times fewer digits to cancellation on images in [0, 1] (measured against float64: the loss 4 to
# 100 times closer, the gradient 4 to 15 times).  The same function, the same gradient.
SHIFT = 0.5


def _pooled(h, w):
    f = max(1, round(min(h, w) / 256))
    return f, h // f, w // f


def _check(x, y):
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"SSIM needs two N x C x H x W images of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    f, hp, wp = _pooled(x.shape[-2], x.shape[-1])
    if hp < KERNEL_SIZE or wp < KERNEL_SIZE:
        raise ValueError(f"SSIM needs a pooled image of at least {KERNEL_SIZE} x {KERNEL_SIZE}, got {hp} x {wp} "
                         f"({x.shape[-2]} x {x.shape[-1]} pooled by {f})")
    return f


def _moments(x, y):
    """G*x', G*y', G*x'x', G*y'y', G*x'y' of x' = x - 1/2, y' = y - 1/2 over the valid map: the Gaussian applied as a row pass and a
    column pass over the five moment planes at once."""
    n, c, h, w = x.shape
    co = torch.arange(KERNEL_SIZE, dtype=x.dtype, device=x.device) - (KERNEL_SIZE - 1) / 2.0
    g = torch.exp(-(co ** 2) / (2 * SIGMA ** 2))
    g = g / g.sum()
    xs, ys = x - SHIFT, y - SHIFT
    z = torch.stack((xs, ys, xs * xs, ys * ys, xs * ys)).reshape(5 * n * c, 1, h, w)
    z = F.conv2d(F.conv2d(z, g.view(1, 1, 1, -1)), g.view(1, 1, -1, 1))
    return z.reshape(5, n, c, h - KERNEL_SIZE + 1, w - KERNEL_SIZE + 1)


def ssim_torch(x, y):
    """SSIM (mean over images, 0-d) of test image `x` against reference `y` in plain torch (fp32 or float64, any device), the
    Gaussian applied as a row pass and a column pass over the five moment planes (of x - 1/2, y - 1/2) at once.  No clamp: `ssim_loss` clamps sr as the
    model does."""
    f = _check(x, y)
    dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    x, y = x.to(dt), y.to(dt)
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    mx, my, xx, yy, xy = _moments(x, y)
    sxx, syy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    mx, my = mx + SHIFT, my + SHIFT
    s = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return s.mean(dim=(-1, -2)).mean(dim=1).mean()


# --------------------------------------------------------------------------------------------
# HIP path (csrc/ssim_loss.hip)
# --------------------------------------------------------------------------------------------
def _args(s, h, *, partial=None, loss=None, gout=None, grad=None):
    n, c, hh, ww = s.shape
    return L.SsimLossArgs(sr=s.data_ptr(), hr=h.data_ptr(), N=n, C=c, H=hh, W=ww, partial=_ptr(partial), loss=_ptr(loss), gout=_ptr(gout),
                          grad=_ptr(grad))


class SSIMLossFn(torch.autograd.Function):
    """1 - SSIM(clamp(sr, 0, 1), hr) as two launches forward (srk_ssim_loss_fwd: clamp, pooling, the separable moments and the
    per-tile sums of the SSIM map; srk_ssim_loss_finalize: the fixed-order reduction and the loss) and one backward
    (srk_ssim_loss_bwd: recomputes each tile's moments from sr and hr on a 10-pixel halo and applies the transposed filter, scaled
    by the upstream gradient read on the device: capturable).  Nothing but sr and hr is kept for the backward."""

    @staticmethod
    def forward(ctx, sr, hr):
        _need_gpu(sr)
        _check(sr, hr)
        s, h = _f32c(sr), _f32c(hr)
        nt = L.load().srk_ssim_loss_tiles(*s.shape)
        if nt <= 0:
            raise ValueError(f"SSIM loss: sizes {tuple(s.shape)} refused")
        partial = torch.empty(nt, dtype=torch.float64, device=s.device)
        loss = torch.empty((), dtype=torch.float32, device=s.device)
        a = _args(s, h, partial=partial, loss=loss)
        L.call("srk_ssim_loss_fwd", a, _stream())
        L.call("srk_ssim_loss_finalize", a, _stream())
        ctx.save_for_backward(s, h)
        return loss

    @staticmethod
    def backward(ctx, g):
        s, h = ctx.saved_tensors
        gout = g.detach().float().contiguous()
        f, hp, wp = _pooled(s.shape[-2], s.shape[-1])
        # the kernel writes the pooled area only: the dropped remainder rows / columns are zeroed here
        grad = torch.empty_like(s) if (hp * f, wp * f) == tuple(s.shape[-2:]) else torch.zeros_like(s)
        L.call("srk_ssim_loss_bwd", _args(s, h, gout=gout, grad=grad), _stream())
        return grad, None


def _hip_ok(sr, hr):
    return (sr.is_cuda and hr.is_cuda and sr.dtype == torch.float32 and hr.dtype == torch.float32 and sr.dim() == 4
            and sr.shape == hr.shape and sr.numel() > 0 and sr.is_contiguous() and hr.is_contiguous())


def ssim_loss(sr, hr):
    """1 - SSIM(clamp(sr, 0, 1), hr): HIP for contiguous CUDA fp32 tensors when `hr` needs no gradient, `ssim_torch` otherwise
    (a strided view goes to the torch statement, which reads it in place, rather than through a hidden copy)."""
    if hr.requires_grad or not _hip_ok(sr, hr):
        return 1.0 - ssim_torch(sr.clamp(0, 1), hr)
    return SSIMLossFn.apply(sr, hr)
