"""MS-SSIM (Wang, Simoncelli, Bovik: "Multiscale structural similarity for image quality assessment", 2003) as a training loss,
1 - MS-SSIM with piq.multi_scale_ssim's defaults (piq.MultiScaleSSIMLoss; the structural term of Zhao et al.'s
"0.16*l1+0.84*ms_ssim"), called like the model's other piq losses on clamp(sr, 0, 1) and hr.  Part of `ops` (re-exported there).

For a test image x = clamp(sr, 0, 1) and a reference y = hr, both N x C x H x W with any C >= 1 and H, W >= 161:
  1. level 0 is (x, y); level k > 0 is level k-1 replicate-padded by p = max(H_{k-1} % 2, W_{k-1} % 2) on the top and left only,
     then averaged 2x2 with stride 2 (floor); no initial pooling (the pyramid of ops.ms_ssim);
  2. per level and (image, channel) plane, cs_k and ss_k are the means over the valid (H_k - 10) x (W_k - 10) map of the
     contrast-structure and SSIM maps (separable 11-tap Gaussian, sigma 1.5, c1 = 1e-4, c2 = 9e-4);
  3. m_k = cs_k (k < 4), m_4 = ss_4; v = prod_k max(m_k, 0)^w_k, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333);
     loss = 1 - mean over images of (mean over channels of v): on in-range input 1 - ops.ms_ssim(x, y).

Gradient: with respect to sr only.  d v / d m_k = w_k v / m_k when every m_k of the plane is positive; a plane with any m_k <= 0
has v = 0 and gets a zero gradient.  The clamp passes the gradient on the closed interval [0, 1] (torch's convention).

Departures and limits, on both paths:
  - piq's relu(m)^w has an infinite slope at m = 0, so its autograd returns NaN for such a plane, and one NaN ruins every
    parameter through Adam: the zero gradient above is deliberate (the policy of flip.py);
  - piq asserts 0 <= y <= 1; that check needs a host sync, which a captured training step cannot do, so hr is not checked;
  - parity with piq itself is not pinned (piq is not a dependency): tests/ms_ssim_loss_ref.py states the definition in float64.
"""
import torch
import torch.nn.functional as F

from . import _lib as L
from .ops import _f32c, _need_gpu, _ptr, _stream      # (ops.py imports this module at its END: these exist by then)
from .ops_metrics import MS_SSIM_WEIGHTS, ms_ssim_check
from .ssim_loss import C1, C2, SHIFT, _hip_ok, _moments      # (ops.py imports ssim_loss before this module)

__all__ = ["ms_ssim_torch", "MSSSIMLossFn", "ms_ssim_loss"]


def ms_ssim_torch(x, y):
    """MS-SSIM (mean over images, 0-d) of test image `x` against reference `y` in plain torch (fp32 or float64, any device),
    differentiable; the Gaussian is a row pass and a column pass over the five moment planes (of x - 1/2, y - 1/2) at once.  A plane
    with a level mean <= 0 has the value 0 and a zero gradient (written with torch.where on a safe base, not relu ** w).  No clamp:
    `ms_ssim_loss` clamps sr as the model does."""
    ms_ssim_check(x, y)
    dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    x, y = x.to(dt), y.to(dt)
    means = []
    last = len(MS_SSIM_WEIGHTS) - 1
    for level in range(last + 1):
        if level > 0:
            p = max(x.shape[-2] % 2, x.shape[-1] % 2)
            x = F.avg_pool2d(F.pad(x, [p, 0, p, 0], mode="replicate"), 2)
            y = F.avg_pool2d(F.pad(y, [p, 0, p, 0], mode="replicate"), 2)
        mx, my, xx, yy, xy = _moments(x, y)
        sxx, syy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
        m = (2 * sxy + C2) / (sxx + syy + C2)
        if level == last:
            mx, my = mx + SHIFT, my + SHIFT
            m = (2 * mx * my + C1) / (mx * mx + my * my + C1) * m
        means.append(m.mean(dim=(-1, -2)))
    m = torch.stack(means)                                             # [5, N, C]
    positive = (m > 0).all(dim=0)
    wt = torch.tensor(MS_SSIM_WEIGHTS, dtype=dt, device=x.device).view(-1, 1, 1)
    safe = torch.where(positive.unsqueeze(0), m, torch.ones_like(m))   # the power never sees a base <= 0: no infinite slope
    v = torch.where(positive, torch.prod(safe ** wt, dim=0), torch.zeros_like(m[0]))
    return v.mean(dim=1).mean()


# --------------------------------------------------------------------------------------------
# HIP path (csrc/ms_ssim_loss.hip)
# --------------------------------------------------------------------------------------------
def _args(s, h, *, workspace=None, partials=None, table=None, loss=None, gout=None, gwork=None, grad=None):
    n, c, hh, ww = s.shape
    return L.MsSsimLossArgs(sr=s.data_ptr(), hr=h.data_ptr(), N=n, C=c, H=hh, W=ww, workspace=_ptr(workspace),
                            partials=_ptr(partials), table=_ptr(table), loss=_ptr(loss), gout=_ptr(gout), gwork=_ptr(gwork),
                            grad=_ptr(grad))


class MSSSIMLossFn(torch.autograd.Function):
    """1 - MS-SSIM(clamp(sr, 0, 1), hr).  Forward: srk_ms_ssim_loss_fwd (the pyramid of both images into a workspace, the clamp
    folded into the reads of level 0, and one launch for the per-tile sums of all five levels' maps), then
    srk_ms_ssim_loss_finalize (the fixed-order reduction, the loss and the per-plane table w_k v / (m_k count_k N C)).  Backward:
    srk_ms_ssim_loss_bwd, one launch per level from the coarsest: recomputes each tile's moments on a 10-pixel halo, applies the
    transposed filter and gathers the parent level's gradient; level 0 scales by the upstream gradient read on the device: capturable.
    sr, hr, the pyramid and the table are kept for the backward."""

    @staticmethod
    def forward(ctx, sr, hr):
        _need_gpu(sr)
        ms_ssim_check(sr, hr)
        s, h = _f32c(sr), _f32c(hr)
        n, c = s.shape[:2]
        lib = L.load()
        tiles = lib.srk_ms_ssim_loss_tiles(*s.shape, None)
        pyr = lib.srk_ms_ssim_loss_workspace_bytes(*s.shape)
        if tiles <= 0 or pyr < 0:
            raise ValueError(f"MS-SSIM loss: sizes {tuple(s.shape)} refused")
        pyramid = torch.empty(pyr // 4, dtype=torch.float32, device=s.device)
        partials = torch.empty(n * c * tiles * 2, dtype=torch.float64, device=s.device)
        table = torch.empty(n * c, len(MS_SSIM_WEIGHTS), dtype=torch.float32, device=s.device)
        loss = torch.empty((), dtype=torch.float32, device=s.device)
        a = _args(s, h, workspace=pyramid, partials=partials, table=table, loss=loss)
        L.call("srk_ms_ssim_loss_fwd", a, _stream())
        L.call("srk_ms_ssim_loss_finalize", a, _stream())
        ctx.save_for_backward(s, h, pyramid, table)
        return loss

    @staticmethod
    def backward(ctx, g):
        s, h, pyramid, table = ctx.saved_tensors
        gout = g.detach().float().contiguous()
        gwork = torch.empty(pyramid.numel() // 2, dtype=torch.float32, device=s.device)      # the gradients of levels 1-4 of sr
        grad = torch.empty_like(s)
        L.call("srk_ms_ssim_loss_bwd", _args(s, h, workspace=pyramid, table=table, gout=gout, gwork=gwork, grad=grad), _stream())
        return grad, None


def ms_ssim_loss(sr, hr):
    """1 - MS-SSIM(clamp(sr, 0, 1), hr): HIP for contiguous CUDA fp32 tensors when `hr` needs no gradient, `ms_ssim_torch` otherwise
    (a strided view goes to the torch statement, which reads it in place, rather than through a hidden copy).  Sides under 161 and
    mismatched or non-4-D shapes raise piq's ValueError, as ops.ms_ssim does."""
    if hr.requires_grad or not _hip_ok(sr, hr):
        return 1.0 - ms_ssim_torch(sr.clamp(0, 1), hr)
    return MSSSIMLossFn.apply(sr, hr)
