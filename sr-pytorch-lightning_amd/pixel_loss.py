"""Pixel-domain training losses beside `l1` and `l2`: Charbonnier, Huber, smooth-L1, Barron's general robust loss with fixed alpha
and c, and the PSNR loss.  Part of `ops` (re-exported there).  csrc/pixel_loss.hip on the GPU, plain torch elsewhere.

With d = sr - hr, mean reduction over every element, and NOTHING clamped (like `l1` the losses take sr as it comes):
  charbonnier(eps=1e-3)   sqrt(d^2 + eps^2): LapSRN's eps; at d = 0 the value is eps, the gradient d / sqrt(d^2 + eps^2) is 0.
                          BasicSR's CharbonnierLoss, sqrt(d^2 + 1e-12), is eps=1e-6 here
  huber(delta=1)          d^2 / 2 if |d| <= delta, else delta (|d| - delta / 2)                    torch.nn.HuberLoss
  smooth_l1(beta=1)       d^2 / (2 beta) if |d| < beta, else |d| - beta / 2; beta = 0 is L1         torch.nn.SmoothL1Loss
  robust(alpha, c)        rho(d; alpha, c) of Barron, "A general and adaptive robust loss function", CVPR 2019, eq. 13, with fixed
                          alpha and c (both required; the learned ones of the reference's `adaptive` entry are out of scope):
                          z = (d / c)^2, b = |alpha - 2|;  alpha = 2: z / 2;  alpha = 0: log1p(z / 2);  alpha = -inf: -expm1(-z / 2);
                          any other finite alpha: (b / alpha) expm1((alpha / 2) log1p(z / b)).  The three exact cases are chosen on the
                          host by comparing alpha with 2, 0 and -inf, never by a tolerance; the fp32 paths compare alpha as fp32
                          holds it (2 - 1e-9 is 2 there), and an alpha fp32 cannot hold (1e-40, 1e39) computes in float64 torch.
                          The expm1 / log1p form is the one every
                          path uses: the textbook (b / alpha) ((z / b + 1)^(alpha / 2) - 1) loses every digit in fp32 at |d| ~ 1e-7
  psnr(eps=1e-8)          NAFNet's PSNRLoss on RGB: (10 / ln 10) mean over images of ln(mse_n + eps), mse_n the mean of d^2 over image
                          n's C H W elements: minus the PSNR in dB, so on in-range images it is -PSNR of the metric table.  An image
                          equal to its target contributes 10 log10(eps) and a zero gradient.

Gradient: with respect to sr only on the HIP path (the entry functions send a target that needs one to the torch path)."""
import ctypes
import math

import torch

from . import _lib as L
from .ops import _f32c, _need_gpu, _stream      # (ops.py imports this module at its END: these exist by then)

__all__ = ["pixel_loss_torch", "psnr_loss_torch", "PixelLossFn", "PSNRLossFn", "charbonnier_loss", "huber_loss", "smooth_l1_loss",
           "robust_loss", "psnr_loss", "PIXEL_LOSS_PARAMS", "pixel_loss_check_params", "pixel_loss_parse_params"]

_REQUIRED = object()
#: loss -> {parameter: default}; `_REQUIRED`: no default
PIXEL_LOSS_PARAMS = {"charbonnier": {"eps": 1e-3}, "huber": {"delta": 1.0}, "smooth_l1": {"beta": 1.0},
                     "robust": {"alpha": _REQUIRED, "c": _REQUIRED}, "psnr": {"eps": 1e-8}}
PSNR_K = 10.0 / math.log(10.0)


def pixel_loss_check_params(name, params):
    """The parameters of loss `name` as floats, defaults filled in and ranges checked: eps, delta and c > 0, beta >= 0, alpha any
    finite float or -inf.  ValueError for an unknown loss or key, a missing required one, and a value that is not a float or is out
    of range."""
    if name not in PIXEL_LOSS_PARAMS:
        raise ValueError(f"pixel loss not recognized: {name!r}. Supported: {', '.join(PIXEL_LOSS_PARAMS)}")
    spec = PIXEL_LOSS_PARAMS[name]
    unknown = sorted(set(params) - set(spec))
    if unknown:
        raise ValueError(f"loss {name!r} has no parameter {', '.join(unknown)} (it takes: {', '.join(spec)})")
    missing = [k for k, v in spec.items() if v is _REQUIRED and k not in params]
    if missing:
        raise ValueError(f"loss {name!r} needs {' and '.join(missing)} (e.g. loss_params=['robust.alpha=-2', 'robust.c=0.05'])")
    out = {}
    for key, default in spec.items():
        v = params.get(key, default)
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"loss {name!r}: {key}={v!r} is not a float") from None
        if key == "alpha":
            ok = not math.isnan(v) and v != math.inf
            rule = "any finite float or -inf"
        elif key == "beta":
            ok, rule = math.isfinite(v) and v >= 0.0, ">= 0"
        else:
            ok, rule = math.isfinite(v) and v > 0.0, "> 0"
        if not ok:
            raise ValueError(f"loss {name!r}: {key}={v} is out of range ({rule})")
        out[key] = v
    return out


def pixel_loss_parse_params(names, entries):
    """`"<loss>.<key>=<value>"` strings -> {loss: checked parameters} for every pixel loss among `names`, e.g.
    ["charbonnier.eps=1e-6", "robust.alpha=-2", "robust.c=0.05"].  ValueError for an entry of another form, one whose loss is not
    in `names`, and everything `pixel_loss_check_params` refuses."""
    given = {}
    for entry in entries:
        left, sep, value = str(entry).strip().partition("=")
        name, dot, key = left.strip().partition(".")
        name, key, value = name.strip().lower(), key.strip(), value.strip()
        if not sep or not dot or not name or not key or not value:
            raise ValueError(f"loss parameter {entry!r} is not <loss>.<key>=<value>")
        if name not in names:
            raise ValueError(f"loss parameter {entry!r}: loss {name!r} is not among the losses ({', '.join(names)})")
        if name not in PIXEL_LOSS_PARAMS:
            raise ValueError(f"loss parameter {entry!r}: loss {name!r} takes no parameters")
        given.setdefault(name, {})[key] = value
    return {name: pixel_loss_check_params(name, given.get(name, {})) for name in names if name in PIXEL_LOSS_PARAMS}


# --------------------------------------------------------------------------------------------
# torch path: the CPU path and the fallback (fp32 or float64, differentiable in both images)
# --------------------------------------------------------------------------------------------
def _diff(sr, hr):
    dt = sr.dtype if sr.dtype in (torch.float32, torch.float64) else torch.float32
    return sr.to(dt) - hr.to(dt)


def _robust(d, alpha, c):
    z = (d / c) ** 2
    if alpha == 2.0:
        return 0.5 * z
    if alpha == 0.0:
        return torch.log1p(0.5 * z)
    if alpha == -math.inf:
        return -torch.expm1(-0.5 * z)
    b = abs(alpha - 2.0)
    return (b / alpha) * torch.expm1((0.5 * alpha) * torch.log1p(z / b))


def pixel_loss_torch(kind, sr, hr, **params):
    """Loss `kind` ("charbonnier", "huber", "smooth_l1", "robust") of sr against hr in plain torch (0-d; float64 inputs stay float64,
    everything else computes in fp32; any device).  Parameters that fp32 cannot hold (`_kind_of` is None: an alpha of 1e-40 or 1e39,
    an eps of 1e-30) compute in float64 and give the fp32 result of that."""
    if kind == "psnr":
        return psnr_loss_torch(sr, hr, **params)
    p = pixel_loss_check_params(kind, params)
    d = _diff(sr, hr)
    if d.dtype == torch.float32 and _kind_of(kind, p) is None:
        return pixel_loss_torch(kind, sr.double(), hr.double(), **p).float()
    if kind == "charbonnier":
        v = torch.sqrt(d * d + p["eps"] ** 2)
    elif kind == "huber":
        ad = d.abs()
        v = torch.where(ad <= p["delta"], 0.5 * d * d, p["delta"] * (ad - 0.5 * p["delta"]))
    elif kind == "smooth_l1":
        ad = d.abs()
        v = ad if p["beta"] == 0.0 else torch.where(ad < p["beta"], 0.5 * d * d / p["beta"], ad - 0.5 * p["beta"])
    else:
        # fp32 arithmetic sees alpha as fp32 holds it, like the kernels: 2 - 1e-9 is the alpha = 2 case there
        v = _robust(d, _f32(p["alpha"]) if d.dtype == torch.float32 else p["alpha"], p["c"])
    return v.mean()


def psnr_loss_torch(sr, hr, eps=1e-8):
    """(10 / ln 10) mean_n ln(mse_n + eps) in plain torch; the first dimension counts the images."""
    eps = pixel_loss_check_params("psnr", {"eps": eps})["eps"]
    d = _diff(sr, hr)
    if d.dtype == torch.float32 and not _normal(eps):            # (an eps fp32 cannot hold: float64, like pixel_loss_torch)
        return psnr_loss_torch(sr.double(), hr.double(), eps).float()
    d = d.reshape(d.shape[0], -1) if d.dim() > 1 else d.reshape(1, -1)
    return PSNR_K * torch.log((d * d).mean(dim=1) + eps).mean()


# --------------------------------------------------------------------------------------------
# HIP path (csrc/pixel_loss.hip)
# --------------------------------------------------------------------------------------------
_FLT_MIN = 2.0 ** -126


def _f32(v):
    """v as the launch arguments carry it: rounded to fp32 (a finite value beyond fp32's range becomes +-inf, one below it 0)."""
    return ctypes.c_float(v).value


def _normal(*values):
    """Every value, rounded to fp32, is a finite, normal, non-zero fp32 number: a constant the kernels can divide by and multiply with
    at full precision."""
    return all(math.isfinite(_f32(v)) and abs(_f32(v)) >= _FLT_MIN for v in values)


def _kind_of(kind, p):
    """(SRK_PIXEL_* id, p0, p1) of a checked parameter set as the kernels will see it, or None when fp32 cannot hold a constant they
    derive from it (eps^2; delta / 2; beta / 2; c^2, 1 / c^2; alpha, b, 1 / b, b / alpha): such parameters take the torch path, which
    then computes in float64.  The parameters are rounded to fp32 FIRST, and the exact robust cases are picked by comparing the
    rounded alpha, the value the kernel gets, with 2, 0 and -inf: 2 - 1e-9 is 2 in fp32 and runs the alpha = 2 kernel, 1e-300 is 0,
    -1e39 is -inf (each within 1e-8 of its own value, relatively); an alpha that is subnormal in fp32, or +inf, is not dispatched."""
    if kind == "charbonnier":
        eps = _f32(p["eps"])
        return (L.SRK_PIXEL_CHARBONNIER, eps, 0.0) if _normal(eps * eps) else None
    if kind == "huber":
        delta = _f32(p["delta"])
        return (L.SRK_PIXEL_HUBER, delta, 0.0) if _normal(0.5 * delta) else None
    if kind == "smooth_l1":
        beta = _f32(p["beta"])
        return (L.SRK_PIXEL_SMOOTH_L1, beta, 0.0) if p["beta"] == 0.0 or _normal(0.5 * beta) else None
    alpha, c = _f32(p["alpha"]), _f32(p["c"])
    if not _normal(c * c) or not _normal(1.0 / _f32(c * c)):
        return None
    if alpha == 2.0:
        return L.SRK_PIXEL_ROBUST_A2, 2.0, c
    if alpha == 0.0:
        return L.SRK_PIXEL_ROBUST_A0, 0.0, c
    if alpha == -math.inf:
        return L.SRK_PIXEL_ROBUST_NEG_INF, 0.0, c
    if not _normal(alpha):
        return None
    b = _f32(abs(alpha - 2.0))
    if not _normal(b) or not _normal(1.0 / b, b / alpha):
        return None
    return L.SRK_PIXEL_ROBUST_GENERAL, alpha, c


def _check_pair(sr, hr):
    if sr.shape != hr.shape:
        raise ValueError(f"the pixel losses need two images of one shape, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    if sr.numel() == 0:
        raise ValueError(f"the pixel losses' HIP path needs at least one element, got {tuple(sr.shape)}")


class PixelLossFn(torch.autograd.Function):
    """apply(sr, hr, kind_id, p0, p1): the mean of an elementwise loss (SRK_PIXEL_*) as two launches forward (srk_pixel_loss_fwd: both
    images read once, one double per block; srk_l1_loss_mean: the fixed-order sum and the division) and one backward
    (srk_pixel_loss_bwd: recomputes the derivative from sr and hr, scaled by the upstream gradient read on the device: capturable).
    Nothing but sr and hr is kept for the backward."""

    @staticmethod
    def forward(ctx, sr, hr, kind_id, p0, p1):
        _need_gpu(sr)
        _need_gpu(hr)
        _check_pair(sr, hr)
        s, h = _f32c(sr), _f32c(hr)
        n = s.numel()
        nb = L.load().srk_pixel_loss_blocks(n)
        partial = torch.empty(nb, dtype=torch.float64, device=s.device)
        out = torch.empty((), dtype=torch.float32, device=s.device)
        a = L.PixelLossArgs(sr=s.data_ptr(), hr=h.data_ptr(), n=n, kind=kind_id, p0=p0, p1=p1, partial=partial.data_ptr(), gout=0,
                            scale=0.0, grad=0)
        L.call("srk_pixel_loss_fwd", a, _stream())
        L.check(L.load().srk_l1_loss_mean(partial.data_ptr(), nb, n, out.data_ptr(), _stream()), "srk_l1_loss_mean")
        ctx.save_for_backward(s, h)
        ctx.kind = (kind_id, p0, p1)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        s, h = ctx.saved_tensors
        kind_id, p0, p1 = ctx.kind
        n = s.numel()
        gout = g.detach().float().contiguous()
        grad = torch.empty_like(s)
        a = L.PixelLossArgs(sr=s.data_ptr(), hr=h.data_ptr(), n=n, kind=kind_id, p0=p0, p1=p1, partial=0, gout=gout.data_ptr(),
                            scale=1.0 / n, grad=grad.data_ptr())
        L.call("srk_pixel_loss_bwd", a, _stream())
        return grad, None, None, None, None


class PSNRLossFn(torch.autograd.Function):
    """apply(sr, hr, eps): the PSNR loss as two launches forward (srk_psnr_loss_fwd: the sums of d^2 per (image, block);
    srk_psnr_loss_finalize: each image's mse, its coefficient and the loss, fixed order) and one backward (srk_psnr_loss_bwd:
    grad = upstream * coef_n * d, the upstream gradient read on the device: capturable).  sr, hr and one float per image are kept."""

    @staticmethod
    def forward(ctx, sr, hr, eps):
        _need_gpu(sr)
        _need_gpu(hr)
        _check_pair(sr, hr)
        s, h = _f32c(sr), _f32c(hr)
        nimg = s.shape[0] if s.dim() > 1 else 1
        per = s.numel() // nimg
        nb = L.load().srk_psnr_loss_blocks(nimg, per)
        if nb <= 0:
            raise ValueError(f"PSNR loss: sizes {tuple(s.shape)} refused")
        partial = torch.empty(nb, dtype=torch.float64, device=s.device)
        coef = torch.empty(nimg, dtype=torch.float32, device=s.device)
        out = torch.empty((), dtype=torch.float32, device=s.device)
        a = L.PsnrLossArgs(sr=s.data_ptr(), hr=h.data_ptr(), N=nimg, per=per, eps=eps, partial=partial.data_ptr(), coef=coef.data_ptr(),
                           loss=out.data_ptr(), gout=0, grad=0)
        L.call("srk_psnr_loss_fwd", a, _stream())
        L.call("srk_psnr_loss_finalize", a, _stream())
        ctx.save_for_backward(s, h, coef)
        ctx.sizes = (nimg, per, eps)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        s, h, coef = ctx.saved_tensors
        nimg, per, eps = ctx.sizes
        gout = g.detach().float().contiguous()
        grad = torch.empty_like(s)
        a = L.PsnrLossArgs(sr=s.data_ptr(), hr=h.data_ptr(), N=nimg, per=per, eps=eps, partial=0, coef=coef.data_ptr(), loss=0,
                           gout=gout.data_ptr(), grad=grad.data_ptr())
        L.call("srk_psnr_loss_bwd", a, _stream())
        return grad, None, None


def _hip_ok(sr, hr):
    """fp32 CUDA tensors of one shape with at least one element, a target that needs no gradient, and contiguous 16-byte-aligned
    storage (the kernels load float4s from the first element: a contiguous view that starts one element into its storage is read in
    place by the torch path instead of through a hidden copy)."""
    return (sr.is_cuda and hr.is_cuda and sr.dtype == torch.float32 and hr.dtype == torch.float32 and sr.shape == hr.shape
            and not hr.requires_grad and sr.numel() > 0 and sr.is_contiguous() and hr.is_contiguous()
            and sr.data_ptr() % 16 == 0 and hr.data_ptr() % 16 == 0)


def _elementwise(kind, sr, hr, params):
    p = pixel_loss_check_params(kind, params)
    launch = _kind_of(kind, p)
    if launch is not None and _hip_ok(sr, hr):
        return PixelLossFn.apply(sr, hr, *launch)
    return pixel_loss_torch(kind, sr, hr, **p)


def charbonnier_loss(sr, hr, eps=1e-3):
    """mean sqrt((sr - hr)^2 + eps^2): HIP when `_hip_ok`, `pixel_loss_torch` otherwise."""
    return _elementwise("charbonnier", sr, hr, {"eps": eps})


def huber_loss(sr, hr, delta=1.0):
    """F.huber_loss(sr, hr, delta=delta): HIP when `_hip_ok`, `pixel_loss_torch` otherwise."""
    return _elementwise("huber", sr, hr, {"delta": delta})


def smooth_l1_loss(sr, hr, beta=1.0):
    """F.smooth_l1_loss(sr, hr, beta=beta) (beta = 0: L1): HIP when `_hip_ok`, `pixel_loss_torch` otherwise."""
    return _elementwise("smooth_l1", sr, hr, {"beta": beta})


def robust_loss(sr, hr, alpha, c):
    """mean rho(sr - hr; alpha, c) of Barron's general robust loss: HIP when `_hip_ok`, `pixel_loss_torch` otherwise."""
    return _elementwise("robust", sr, hr, {"alpha": alpha, "c": c})


def psnr_loss(sr, hr, eps=1e-8):
    """(10 / ln 10) mean_n ln(mse_n + eps), minus the PSNR in dB: HIP when `_hip_ok`, `psnr_loss_torch` otherwise."""
    eps = pixel_loss_check_params("psnr", {"eps": eps})["eps"]
    if _normal(eps) and _hip_ok(sr, hr) and L.load().srk_psnr_loss_blocks(sr.shape[0] if sr.dim() > 1 else 1, sr[0].numel() if sr.dim() > 1 else sr.numel()) > 0:
        return PSNRLossFn.apply(sr, hr, _f32(eps))
    return psnr_loss_torch(sr, hr, eps)
