"""HaarPSI (Reisenhofer, Bosse, Kutyniok, Wiegand: "A Haar wavelet-based perceptual similarity index for image quality
assessment", 2018) as a training loss, with piq 0.7.0's `haarpsi` / `HaarPSILoss` defaults (reference srmodel.py:36, which
calls it on clamp(sr, 0, 1) and hr).  Part of `ops` (re-exported there).

For a test image x = clamp(sr, 0, 1) and a reference y = hr, both N x C x H x W with H, W >= 16:
  1. both x255; C == 3: YIQ per pixel (piq's rgb2yiq), otherwise channel 0 is Y and there is no colour term;
  2. subsampled: zero pad p = max(H % 2, W % 2) rows / columns at the bottom / right, 2x2 / stride-2 mean;
  3. Haar coefficients of Y' at k = 2, 4, 8: zero pad k/2 - 1 top / left and k/2 bottom / right, cross-correlation with
     K0[a, b] = +1/k (a < k/2), -1/k (a >= k/2) and K1 = K0^T;
  4. w_o = max(|h_8^o x|, |h_8^o y|), sim_o = (S(|h_2^o x|, |h_2^o y|) + S(|h_4^o x|, |h_4^o y|)) / 2 for o = 0, 1 with
     S(u, v) = (2uv + c) / (u^2 + v^2 + c + EPS), c = 30, EPS = 2^-23;
  5. C == 3: I', Q' zero padded by one at the bottom / right and 2x2 / stride-1 averaged; sim_2 = (S(i) + S(q)) / 2 and
     w_2 = (w_0 + w_1) / 2;
  6. r_n = (sum sigma(alpha sim) w + eps) / (sum w + eps), alpha = 4.2, eps = 2^-23; h_n = (logit(r_n) / alpha)^2;
     index = mean h_n, loss = 1 - index.

Gradient: with respect to sr only, with torch's conventions (abs at 0: 0; maximum on a tie: half to each side; the clamp
passes the gradient on the closed interval [0, 1]).

Departures and limits, on both paths:
  - piq asserts 0 <= y <= 1; that check needs a host sync, which a captured training step cannot do, so hr is not checked;
  - if the Y planes of both images are all zero every weight is 0, r = 1 and the loss is -inf (the torch statement gives the
    same); it is not special-cased;
  - parity with piq itself is not pinned (piq is not a dependency): tests/haarpsi_ref.py states the definition in float64.
"""
import torch
import torch.nn.functional as F

from . import _lib as L
from .ops import _f32c, _need_gpu, _ptr, _stream      # (ops.py imports this module at its END: these exist by then)

__all__ = ["haarpsi_torch", "HaarPSILossFn", "haarpsi_loss", "haarpsi"]

C_CONST, ALPHA, EPS = 30.0, 4.2, 2.0 ** -23
_YIQ = ((0.299, 0.587, 0.114), (0.5959, -0.2746, -0.3213), (0.2115, -0.5227, 0.3112))
MIN_SIZE = 16                   # piq: 2 ** (scales + 1)


def _check(x, y):
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"HaarPSI needs two N x C x H x W images of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[-2] < MIN_SIZE or x.shape[-1] < MIN_SIZE:
        raise ValueError(f"HaarPSI needs H, W >= {MIN_SIZE}, got {x.shape[-2]} x {x.shape[-1]}")


def _sim(u, v):
    return (2.0 * u * v + C_CONST) / (u * u + v * v + C_CONST + EPS)


def _box(t, k, vertical_sign):
    """Haar response of scale k (cross-correlation, zero pad k/2 - 1 before and k/2 after) as a k x k box: the (upper - lower)
    difference of k-wide row sums when vertical_sign, else the (left - right) difference of k-tall column sums."""
    h = k // 2
    t = F.pad(t, (h - 1, h, h - 1, h))
    rows = F.avg_pool2d(t, (1, k), stride=1) * k if vertical_sign else F.avg_pool2d(t, (k, 1), stride=1) * k
    if vertical_sign:                                      # rows: (H + k - 1) x W -> upper k/2 minus lower k/2
        up = F.avg_pool2d(rows[..., : rows.shape[-2] - h, :], (h, 1), stride=1) * h
        lo = F.avg_pool2d(rows[..., h:, :], (h, 1), stride=1) * h
    else:
        up = F.avg_pool2d(rows[..., : rows.shape[-1] - h], (1, h), stride=1) * h
        lo = F.avg_pool2d(rows[..., h:], (1, h), stride=1) * h
    return (up - lo) / k


def haarpsi_torch(x, y):
    """HaarPSI index (mean over images, 0-d) of test image `x` against reference `y` in plain torch (fp32 or float64, any
    device).  No clamp: `haarpsi_loss` clamps sr as the model does."""
    _check(x, y)
    dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    x, y = x.to(dt) * 255.0, y.to(dt) * 255.0
    n = x.shape[0]
    rgb = x.shape[1] == 3
    z = torch.cat((x, y), 0)
    if rgb:
        m = torch.tensor(_YIQ, dtype=dt, device=z.device)
        z = torch.einsum("ij,njhw->nihw", m, z)
    else:
        z = z[:, :1]
    p = max(x.shape[2] % 2, x.shape[3] % 2)
    z = F.avg_pool2d(F.pad(z, (0, p, 0, p)), 2, stride=2)
    yc = z[:, :1]
    hv = [_box(yc, k, True) for k in (2, 4, 8)]
    hh = [_box(yc, k, False) for k in (2, 4, 8)]
    ws, sims = [], []
    for h in (hv, hh):
        a = [t.abs() for t in h]
        ws.append(torch.maximum(a[2][:n], a[2][n:]))
        sims.append(0.5 * (_sim(a[0][:n], a[0][n:]) + _sim(a[1][:n], a[1][n:])))
    if rgb:
        iq = F.avg_pool2d(F.pad(z[:, 1:], (0, 1, 0, 1)), 2, stride=1).abs()
        sims.append(0.5 * (_sim(iq[:n, 0:1], iq[n:, 0:1]) + _sim(iq[:n, 1:2], iq[n:, 1:2])))
        ws.append(0.5 * (ws[0] + ws[1]))
    w = torch.cat(ws, 1)
    s = torch.cat(sims, 1)
    r = ((torch.sigmoid(ALPHA * s) * w).sum(dim=(1, 2, 3)) + EPS) / (w.sum(dim=(1, 2, 3)) + EPS)
    return ((torch.log(r / (1.0 - r)) / ALPHA) ** 2).mean()


# --------------------------------------------------------------------------------------------
# HIP path (csrc/haarpsi.hip)
# --------------------------------------------------------------------------------------------
def _args(s, h, *, partial, planes, stats, loss=None, index=None, gout=None, grad=None):
    n, c, hh, ww = s.shape
    return L.HaarpsiArgs(sr=s.data_ptr(), hr=_ptr(h), N=n, C=c, H=hh, W=ww, partial=_ptr(partial), planes=_ptr(planes),
                         stats=_ptr(stats), loss=_ptr(loss), index=_ptr(index), gout=_ptr(gout), grad=_ptr(grad))


def _forward(sr, hr, want_index, want_planes):
    """Forward + finalize: (loss, index or None, sr, partial, planes or None, stats) on the device, no host sync.  `planes`: the
    subsampled Y' (and I', Q') planes of both images, which the backward reads."""
    _need_gpu(sr)
    _check(sr, hr)
    s, h = _f32c(sr), _f32c(hr)
    n, c, hh, ww = s.shape
    if c not in (1, 3):
        raise ValueError(f"the HIP HaarPSI takes C = 1 or 3, got {c}")
    nt = L.load().srk_haarpsi_tiles(n, hh, ww)
    if nt <= 0:
        raise ValueError(f"HaarPSI: sizes {tuple(s.shape)} refused")
    partial = torch.empty(2 * nt, dtype=torch.float64, device=s.device)
    stats = torch.empty(n, 4, dtype=torch.float32, device=s.device)
    p = max(hh % 2, ww % 2)
    planes = torch.empty(n, 6 if c == 3 else 2, (hh + p) // 2, (ww + p) // 2, dtype=torch.float32, device=s.device) if want_planes else None
    loss = torch.empty((), dtype=torch.float32, device=s.device)
    index = torch.empty((), dtype=torch.float32, device=s.device) if want_index else None
    a = _args(s, h, partial=partial, planes=planes, stats=stats, loss=loss, index=index)
    L.call("srk_haarpsi_fwd", a, _stream())
    L.call("srk_haarpsi_finalize", a, _stream())
    return loss, index, s, partial, planes, stats


class HaarPSILossFn(torch.autograd.Function):
    """1 - HaarPSI(clamp(sr, 0, 1), hr) as two launches forward (srk_haarpsi_fwd: both images, the Haar coefficients and the
    per-tile sums, keeping the subsampled planes; srk_haarpsi_finalize: the fixed-order per-image reduction and the loss) and one
    backward (srk_haarpsi_bwd: recomputes the tile's coefficients from the planes and applies the chain rule down to sr, scaled by
    the upstream gradient read on the device: capturable).
    The clamp happens inside the kernels."""

    @staticmethod
    def forward(ctx, sr, hr):
        loss, _, s, partial, planes, stats = _forward(sr, hr, False, ctx.needs_input_grad[0])
        ctx.save_for_backward(s, partial, planes, stats)
        return loss

    @staticmethod
    def backward(ctx, g):
        s, partial, planes, stats = ctx.saved_tensors
        gout = g.detach().float().contiguous()
        grad = torch.empty_like(s)
        L.call("srk_haarpsi_bwd", _args(s, None, partial=partial, planes=planes, stats=stats, gout=gout, grad=grad), _stream())
        return grad, None


def _hip_ok(sr, hr):
    return (sr.is_cuda and sr.dtype == torch.float32 and hr.dtype == torch.float32 and sr.dim() == 4 and sr.shape[1] in (1, 3)
            and sr.shape == hr.shape and sr.numel() > 0)


def haarpsi_loss(sr, hr):
    """1 - HaarPSI(clamp(sr, 0, 1), hr): HIP for CUDA fp32 tensors with C in {1, 3} when `hr` needs no gradient,
    `haarpsi_torch` otherwise."""
    if hr.requires_grad or not _hip_ok(sr, hr):
        return 1.0 - haarpsi_torch(sr.clamp(0, 1), hr)
    return HaarPSILossFn.apply(sr, hr)


def haarpsi(x, y):
    """HaarPSI index of clamp(x, 0, 1) against `y` as a 0-d tensor, no gradient (no host sync on the GPU): 1 - haarpsi_loss."""
    with torch.no_grad():
        if not _hip_ok(x, y):
            return haarpsi_torch(x.clamp(0, 1), y)
        return _forward(x, y, True, False)[1]
