"""Frequency-domain training losses: `fft` (BasicSR's FFTLoss, the term of NAFSSR's and MIMO-UNet's `l1 + 0.01..0.1 * fft`) and `ffl`
(the focal frequency loss of Jiang, Dai, Wu, Loy, ICCV 2021).  Part of `ops` (re-exported there).  csrc/freq_loss.hip on the GPU, plain
torch elsewhere.

With d = sr - hr, NOTHING clamped (like `l1`), per plane (n, c) of H x W:
  D[k, l] = sum_{h, w} d[h, w] e^{-2 pi i (k h / H + l w / W)}: the full spectrum, unnormalised (torch.fft.fft2's).
  At the self-conjugate bins (2k = 0 mod H and 2l = 0 mod W) Im D IS 0, because d is real: every path sets it to 0 and never keeps a
  rounding residue there; its sign is 0 in the gradient.

  fft              BasicSR FFTLoss: fft2, stack(real, imag), L1 mean: L = (sum |Re D| + sum |Im D|) / (2 N C H W).  No parameters.
                   UNNORMALISED like BasicSR's: |D| grows with sqrt(H W) for noise-like d, so a weight tuned at one patch size scales
                   with sqrt(H W) at another.  Gradient: Re(F^H G) / (2 N C H W), G = sign(Re D) + i sign(Im D).
  ffl(alpha=1)     FocalFrequencyLoss with patch_factor=1, ave_spectrum=False, log_matrix=False, batch_matrix=False:
                   Do = D / sqrt(H W), q = |Do|^2, w = (q / q_max)^(alpha / 2) with q_max the plane's maximum, w a CONSTANT of the
                   gradient; L = sum w q / (N C H W).  A plane with q_max = 0 gets w = 0: loss 0, gradient 0 (the original's
                   NaN -> 0 line).  alpha = 0 is mse(sr, hr) (Parseval).  alpha is a float >= 0.

Gradient: with respect to sr only on the HIP path (the entry functions send a target that needs one to the torch path).  The HIP path
takes fp32 contiguous N x C x H x W CUDA tensors with 1 <= H, W <= 512 and, for ffl, alpha <= 8; everything else computes in torch."""
import math

import torch

from . import _lib as L
from .ops import _f32c, _need_gpu, _ptr, _stream      # (ops.py imports this module at its END: these exist by then)

__all__ = ["fft_loss_torch", "ffl_loss_torch", "FFTLossFn", "FFLLossFn", "fft_loss", "ffl_loss", "FREQ_LOSS_PARAMS",
           "ffl_check_alpha", "freq_loss_parse_params"]

#: loss -> {parameter: default}
FREQ_LOSS_PARAMS = {"ffl": {"alpha": 1.0}}
MAX_SIZE = L.SRK_FREQ_MAX_SIZE
MAX_ALPHA = float(L.SRK_FREQ_MAX_ALPHA)


def ffl_check_alpha(alpha):
    """alpha as a float; ValueError unless it is a finite float >= 0."""
    try:
        v = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"loss 'ffl': alpha={alpha!r} is not a float") from None
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"loss 'ffl': alpha={v} is out of range (a finite float >= 0)")
    return v


def freq_loss_parse_params(entries):
    """`"ffl.<key>=<value>"` strings -> {"ffl": {"alpha": checked float}}, the default filled in.  ValueError for an entry of another
    form, a key `ffl` does not have, and an alpha `ffl_check_alpha` refuses."""
    given = {}
    for entry in entries:
        left, sep, value = str(entry).strip().partition("=")
        name, dot, key = left.strip().partition(".")
        name, key, value = name.strip().lower(), key.strip(), value.strip()
        if not sep or not dot or name != "ffl" or not key or not value:
            raise ValueError(f"loss parameter {entry!r} is not ffl.<key>=<value>")
        if key not in FREQ_LOSS_PARAMS["ffl"]:
            raise ValueError(f"loss 'ffl' has no parameter {key} (it takes: {', '.join(FREQ_LOSS_PARAMS['ffl'])})")
        given[key] = value
    return {"ffl": {"alpha": ffl_check_alpha(given.get("alpha", FREQ_LOSS_PARAMS["ffl"]["alpha"]))}}


def _check(sr, hr):
    if sr.dim() != 4 or sr.shape != hr.shape:
        raise ValueError(f"the frequency losses need two N x C x H x W images of one shape, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    if sr.numel() == 0:
        raise ValueError(f"the frequency losses need non-empty images, got {tuple(sr.shape)}")


def _twiddles(n):
    """cos and sin of 2 pi m / n, m = 0 .. n - 1, in float64 ([2][n])."""
    ang = 2.0 * math.pi * torch.arange(n, dtype=torch.float64) / n
    return torch.stack((torch.cos(ang), torch.sin(ang)))


# --------------------------------------------------------------------------------------------
# torch path: the CPU path and the fallback (fp32 or float64, differentiable in both images)
# --------------------------------------------------------------------------------------------
_matrices = {}


def _dft_matrices(n, dtype, device):
    """(C, S)[j, k] = cos, sin(2 pi ((j k) mod n) / n): the integer product reduced exactly, the angle in float64, rounded once."""
    key = (n, dtype, str(device))
    m = _matrices.get(key)
    if m is None:
        j = torch.arange(n, dtype=torch.int64)
        tw = _twiddles(n)[:, (j[:, None] * j[None, :]) % n]
        m = _matrices[key] = tw.to(dtype).to(device)        # (under a graph capture the first call must have happened before)
    return m[0], m[1]


def _spectrum(sr, hr):
    """(Re D, Im D) of d = sr - hr as matrix products, Im D set to 0 at the self-conjugate bins."""
    _check(sr, hr)
    dt = sr.dtype if sr.dtype in (torch.float32, torch.float64) else torch.float32
    d = sr.to(dt) - hr.to(dt)
    H, W = d.shape[-2:]
    ch, sh = _dft_matrices(H, dt, d.device)
    cw, sw = _dft_matrices(W, dt, d.device)
    tr, ti = ch @ d, -(sh @ d)
    re, im = tr @ cw + ti @ sw, ti @ cw - tr @ sw
    k, l = torch.arange(H, device=d.device), torch.arange(W, device=d.device)
    structural = ((2 * k) % H == 0)[:, None] & ((2 * l) % W == 0)[None, :]
    return re, im.masked_fill(structural, 0.0)


def fft_loss_torch(sr, hr):
    """(sum |Re D| + sum |Im D|) / (2 N C H W) in plain torch (0-d; float64 inputs stay float64, everything else computes in fp32)."""
    re, im = _spectrum(sr, hr)
    return (re.abs().sum() + im.abs().sum()) / (2 * re.numel())


def ffl_loss_torch(sr, hr, alpha=1.0):
    """The focal frequency loss in plain torch (0-d; float64 inputs stay float64, everything else computes in fp32)."""
    alpha = ffl_check_alpha(alpha)
    re, im = _spectrum(sr, hr)
    q = (re * re + im * im) / (re.shape[-2] * re.shape[-1])
    with torch.no_grad():
        qmax = q.amax(dim=(-2, -1), keepdim=True)
        live = qmax > 0
        w = torch.where(live, (q / torch.where(live, qmax, torch.ones_like(qmax))) ** (0.5 * alpha), torch.zeros_like(q))
    return (w * q).sum() / q.numel()


# --------------------------------------------------------------------------------------------
# HIP path (csrc/freq_loss.hip)
# --------------------------------------------------------------------------------------------
_dev_twiddles = {}


def _twiddles_for(n, device):
    """The fp32 [2][n] twiddle table of size n on `device`, built once per size and cached (a replayed graph reads the same
    allocation)."""
    key = (n, device.index if device.index is not None else torch.cuda.current_device())
    tab = _dev_twiddles.get(key)
    if tab is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the twiddle tables are built on the first eager call; call the loss once before capturing a graph")
        tab = _dev_twiddles[key] = _twiddles(n).float().to(torch.device("cuda", key[1])).contiguous()
    return tab


class _FreqLossFn(torch.autograd.Function):
    """Two entry points forward (srk_*_loss_fwd: sr and hr read once per block of 32 spectrum rows, the transform on the fp32 matrix
    pipe, the elementwise term on the accumulators, two doubles per workgroup; srk_*_loss_finalize: the fixed-order sums and the loss)
    and one backward (srk_*_loss_bwd, two launches: the spectrum recomputed, G formed in place and transformed along the rows into an
    image-sized scratch buffer; then the adjoint along the columns times the upstream gradient read on the device: capturable), which
    writes every element of the gradient.  Nothing but sr, hr (and one float per plane for ffl) is kept for the backward."""
    NAME = None

    @classmethod
    def _args(cls, s, h, alpha, **ptrs):
        n, c, hh, ww = s.shape
        fields = dict(sr=s.data_ptr(), hr=h.data_ptr(), N=n, C=c, H=hh, W=ww, tw_h=_twiddles_for(hh, s.device).data_ptr(),
                      tw_w=_twiddles_for(ww, s.device).data_ptr(), **{k: _ptr(v) for k, v in ptrs.items()})
        if cls.NAME == "ffl":
            return L.FflLossArgs(alpha=alpha, **fields)
        del fields["qmax"]                               # (srk_fft_loss_args has neither alpha nor qmax)
        return L.FftLossArgs(**fields)

    @classmethod
    def _forward(cls, ctx, sr, hr, alpha):
        _need_gpu(sr)
        _need_gpu(hr)
        _check(sr, hr)
        s, h = _f32c(sr), _f32c(hr)
        nt = L.load().srk_freq_loss_tiles(*s.shape)
        if nt <= 0:
            raise ValueError(f"{cls.NAME} loss: sizes {tuple(s.shape)} refused (1 <= H, W <= {MAX_SIZE})")
        partial = torch.empty(nt, 2, dtype=torch.float64, device=s.device)
        qmax = torch.empty(s.shape[0] * s.shape[1], dtype=torch.float32, device=s.device)
        loss = torch.empty((), dtype=torch.float32, device=s.device)
        a = cls._args(s, h, alpha, partial=partial, qmax=qmax, loss=loss, scratch=None, gout=None, grad=None)
        L.call(f"srk_{cls.NAME}_loss_fwd", a, _stream())
        L.call(f"srk_{cls.NAME}_loss_finalize", a, _stream())
        ctx.save_for_backward(s, h, qmax)
        ctx.alpha = alpha
        return loss

    @classmethod
    def _backward(cls, ctx, g):
        s, h, qmax = ctx.saved_tensors
        gout = g.detach().float().contiguous()
        grad = torch.empty_like(s)                       # the second launch writes every element
        n, c, hh, ww = s.shape
        scratch = torch.empty(n * c, 2, hh // 2 + 1, ww, dtype=torch.float32, device=s.device)
        a = cls._args(s, h, ctx.alpha, partial=None, qmax=qmax, loss=None, scratch=scratch, gout=gout, grad=grad)
        L.call(f"srk_{cls.NAME}_loss_bwd", a, _stream())
        return grad


class FFTLossFn(_FreqLossFn):
    """apply(sr, hr): the FFT loss on the HIP path (see `_FreqLossFn`)."""
    NAME = "fft"

    @staticmethod
    def forward(ctx, sr, hr):
        return FFTLossFn._forward(ctx, sr, hr, 0.0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return FFTLossFn._backward(ctx, g), None


class FFLLossFn(_FreqLossFn):
    """apply(sr, hr, alpha): the focal frequency loss on the HIP path (see `_FreqLossFn`); 0 <= alpha <= 8."""
    NAME = "ffl"

    @staticmethod
    def forward(ctx, sr, hr, alpha):
        return FFLLossFn._forward(ctx, sr, hr, float(alpha))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return FFLLossFn._backward(ctx, g), None, None


def _hip_ok(sr, hr):
    """fp32 contiguous CUDA tensors N x C x H x W of one shape, 1 <= H, W <= 512, and a target that needs no gradient."""
    return (sr.is_cuda and hr.is_cuda and sr.dtype == torch.float32 and hr.dtype == torch.float32 and sr.dim() == 4
            and sr.shape == hr.shape and sr.numel() > 0 and not hr.requires_grad and sr.is_contiguous() and hr.is_contiguous()
            and sr.shape[-2] <= MAX_SIZE and sr.shape[-1] <= MAX_SIZE)


def fft_loss(sr, hr):
    """BasicSR's FFTLoss of sr against hr: HIP when `_hip_ok`, `fft_loss_torch` otherwise (other dtypes, strided views, planes
    larger than 512, a target that needs a gradient, CPU tensors)."""
    _check(sr, hr)
    if _hip_ok(sr, hr):
        return FFTLossFn.apply(sr, hr)
    return fft_loss_torch(sr, hr)


def ffl_loss(sr, hr, alpha=1.0):
    """The focal frequency loss of sr against hr: HIP when `_hip_ok` and alpha <= 8, `ffl_loss_torch` otherwise."""
    alpha = ffl_check_alpha(alpha)
    _check(sr, hr)
    if _hip_ok(sr, hr) and alpha <= MAX_ALPHA:
        return FFLLossFn.apply(sr, hr, alpha)
    return ffl_loss_torch(sr, hr, alpha)
