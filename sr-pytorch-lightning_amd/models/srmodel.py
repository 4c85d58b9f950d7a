"""`SRModel`: the reference's LightningModule base, restated for the MI355X build.

Mirrors models/srmodel.py:67-621 of the reference for the part of the surface the hot
path needs: constructor keywords, `forward` (abstract), `training_step`,
`validation_step`, `predict_step`, `configure_optimizers`, the loss-string parser and the
metric table.  Lightning is optional: when `lightning.pytorch` is importable the class
derives from `LightningModule` (so the reference's `main.py` / Trainer can drive it);
otherwise from `nn.Module` with no-op logging hooks and `trainer.py`'s own fit loop.

Out of scope: the learned perceptual losses (lpips, dists,
pieapp; `vgg` is built: vgg_loss.py) and the adaptive one, Comet / TensorBoard image dumps, model-parallel flags (accepted and ignored with a warning).
"""
import contextlib
import functools
import itertools
import logging
from dataclasses import dataclass
from typing import Any, Callable

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ema as _ema
from .. import grad_accum as _grad_accum
from .. import grad_clip as _grad_clip
from .. import lr_sched as _lr_sched
from .. import optim as _hip_optim
from .. import tiling as _tiling

try:  # pragma: no cover - lightning is not installed in the build image
    import lightning.pytorch as pl
    _Base = pl.LightningModule
    HAVE_LIGHTNING = True
except Exception:  # noqa: BLE001
    HAVE_LIGHTNING = False

    class _Base(nn.Module):
        """Minimal stand-in for LightningModule (bookkeeping only)."""

        def save_hyperparameters(self, *a, **k):
            pass

        def log_dict(self, *a, **k):
            pass

        def log(self, *a, **k):
            pass

        @property
        def device(self):
            try:
                return next(self.parameters()).device
            except StopIteration:
                return torch.device("cpu")


@dataclass
class _SubLoss:
    name: str
    loss: Callable
    weight: float = 1.0


# models/srmodel.py:30-44 -- only the torch-native entries are on the path
def _l1_loss(sr, hr):
    """F.l1_loss; on the GPU the fused HIP forward/backward pair (ops.L1LossFn)."""
    if sr.is_cuda and sr.dtype == torch.float32 and sr.shape == hr.shape:
        from .. import ops
        return ops.l1_loss(sr, hr)
    return F.l1_loss(sr, hr)


def _flip_loss(sr, hr):
    """FLIPLoss (losses/flip.py, srmodel.py:35): mean FLIP error of sr against hr; on the GPU the fused HIP forward/backward
    (flip.FlipLossFn), elsewhere flip.flip_torch.  Finite gradients everywhere (flip.py: the reference's are NaN where the two
    images' filtered colours coincide)."""
    from .. import flip
    return flip.flip_loss(sr, hr)


def _haarpsi_loss(sr, hr):
    """piq.HaarPSILoss (srmodel.py:36), called as the reference does on clamp(sr, 0, 1) and hr (srmodel.py:525-528): 1 - HaarPSI;
    on the GPU the fused HIP forward/backward (haarpsi.HaarPSILossFn, which clamps inside), elsewhere haarpsi.haarpsi_torch."""
    from .. import haarpsi
    return haarpsi.haarpsi_loss(sr, hr)


def _ssim_loss(sr, hr):
    """piq.SSIMLoss with piq.ssim's defaults, called like the other piq losses on clamp(sr, 0, 1) and hr: 1 - SSIM, the structural
    term of "0.16*l1+0.84*ssim" (Zhao et al. 2017); on the GPU the fused HIP forward/backward (ssim_loss.SSIMLossFn, which clamps
    inside), elsewhere ssim_loss.ssim_torch.  On in-range images the value is 1 - _ssim(sr, hr)."""
    from .. import ssim_loss
    return ssim_loss.ssim_loss(sr, hr)


def _ms_ssim_loss(sr, hr):
    """piq.MultiScaleSSIMLoss with piq.multi_scale_ssim's defaults, called like the other piq losses on clamp(sr, 0, 1) and hr:
    1 - MS-SSIM, the structural term of "0.16*l1+0.84*ms_ssim" (Zhao et al. 2017); on the GPU the fused HIP forward/backward
    (ms_ssim_loss.MSSSIMLossFn, which clamps inside), elsewhere ms_ssim_loss.ms_ssim_torch.  Needs an HR patch of at least 161."""
    from .. import ms_ssim_loss
    return ms_ssim_loss.ms_ssim_loss(sr, hr)


def _gmsd_loss(sr, hr):
    """piq.GMSDLoss (gradient magnitude similarity deviation), called like the other piq losses on clamp(sr, 0, 1) and hr: the
    deviation itself, 0 for a perfect match; the edge-aware term that, unlike the reference's `edge_loss`, carries a gradient.  On the
    GPU the fused HIP forward/backward (gmsd.GMSDLossFn, which clamps inside), elsewhere gmsd.gmsd_torch.  1 or 3 channels."""
    from .. import gmsd
    return gmsd.gmsd_loss(sr, hr)


def _pixel_loss(name):
    """The pixel losses of pixel_loss.py (BasicSR's CharbonnierLoss and PSNRLoss, torch's HuberLoss and SmoothL1Loss, Barron's robust
    loss with fixed alpha and c), called on sr as it comes (no clamp, like l1): fn(sr, hr, **parameters); on the GPU the fused HIP
    forward/backward (pixel_loss.PixelLossFn / PSNRLossFn), elsewhere pixel_loss.pixel_loss_torch.  `_create_losses` binds the
    parameters that `loss_params` gives."""
    def fn(sr, hr, **params):
        from .. import pixel_loss
        return getattr(pixel_loss, f"{name}_loss")(sr, hr, **params)
    fn.__name__ = f"_{name}_loss"
    return fn


def _fft_loss(sr, hr):
    """BasicSR's FFTLoss (the L1 of the 2-D spectrum; NAFSSR's and MIMO-UNet's `l1 + 0.01..0.1 * fft`), called on sr as it comes
    (no clamp, like l1).  UNNORMALISED like BasicSR's: its weight scales with sqrt(H W) of the HR patch.  On the GPU the fused HIP
    forward/backward (freq_loss.FFTLossFn), elsewhere freq_loss.fft_loss_torch."""
    from .. import freq_loss
    return freq_loss.fft_loss(sr, hr)


def _ffl_loss(sr, hr, **params):
    """The focal frequency loss (Jiang et al., ICCV 2021; patch_factor=1, no averaging, no log), called on sr as it comes;
    `loss_params` gives `ffl.alpha` (default 1).  On the GPU the fused HIP forward/backward (freq_loss.FFLLossFn), elsewhere
    freq_loss.ffl_loss_torch."""
    from .. import freq_loss
    return freq_loss.ffl_loss(sr, hr, **params)


def _vgg_loss(sr, hr, **params):
    """VGGLoss (losses/losses.py:54-117; the reference's commented `'vgg'` hook): rescale * the MSE (or L1) between the features of a
    FROZEN VGG-19 / VGG-16 slice of sr as it comes (no clamp) and of hr.  `loss_params` gives `vgg.weights` (required: a state-dict
    file; nothing is downloaded), `vgg.net`, `vgg.layer`, `vgg.rescale`, `vgg.criterion`, `vgg.precision`.  `_create_losses` puts a
    `vgg_loss.VGGLoss` that owns the weights in this function's place; called directly it builds one per call.  On the GPU the HIP
    feature stack (vgg_loss.VGGLossFn), elsewhere vgg_loss.vgg_loss_torch."""
    from .. import vgg_loss
    return vgg_loss.VGGLoss(**params)(sr, hr)


_pixel_losses = ("charbonnier", "huber", "smooth_l1", "robust", "psnr")
_supported_losses = {"l1": _l1_loss, "l2": F.mse_loss, "mae": _l1_loss, "mse": F.mse_loss, "flip": _flip_loss,
                     "haarpsi": _haarpsi_loss, "ssim": _ssim_loss, "ms_ssim": _ms_ssim_loss, "gmsd": _gmsd_loss,
                     **{name: _pixel_loss(name) for name in _pixel_losses}, "vgg": _vgg_loss, "fft": _fft_loss, "ffl": _ffl_loss}
_MS_SSIM_MIN_PATCH = 161          # ops_metrics.MS_SSIM_MIN_SIZE: (11 - 1) * 2^4 + 1
_out_of_scope_losses = {"adaptive", "dists", "edge_loss", "lpips", "pencil_sketch", "pieapp"}

# models/srmodel.py:57-64
# 'ADAM', 'RMSprop' and 'SGD' are torch.optim.Adam / RMSprop / SGD and 'Ranger' is torch_optimizer.Ranger, each with the update of
# GPU parameters as one HIP launch (sr-pytorch-lightning_amd/optim.py; CPU parameters step through the torch classes
# themselves); RangerVA and RangerQH are not built
_supported_optimizers = {"ADAM": _hip_optim.Adam, "Ranger": _hip_optim.Ranger, "RMSprop": _hip_optim.RMSprop, "SGD": _hip_optim.SGD}
_out_of_scope_optimizers = {"RangerVA", "RangerQH"}


def _psnr(x, y):
    """RGB PSNR, data_range 1, per image then batch mean (piq.psnr defaults; srmodel.py:52,582).
    On the GPU the squared-error reduction is the HIP kernel srk_image_sse (no D2H sync per image)."""
    if x.is_cuda:
        from .. import ops
        return ops.psnr(x, y)
    mse = ((x.float() - y.float()) ** 2).flatten(1).mean(dim=1)
    return (10.0 * torch.log10(1.0 / (mse + 1e-8))).mean()


def _ssim(x, y, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """SSIM with piq.ssim's defaults (11x11 Gaussian, sigma 1.5, avg-pool by round(min(H,W)/256)).
    On the GPU: the HIP reduction srk_image_ssim."""
    if x.is_cuda and kernel_size == 11:
        from .. import ops
        return ops.ssim(x, y, sigma=sigma, k1=k1, k2=k2)
    x, y = x.float(), y.float()
    f = max(1, round(min(x.shape[-2:]) / 256))
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    c = x.shape[1]
    co = torch.arange(kernel_size, dtype=torch.float32, device=x.device) - (kernel_size - 1) / 2.0
    g = torch.exp(-(co ** 2) / (2 * sigma ** 2))
    g = g / g.sum()
    k = torch.outer(g, g).view(1, 1, kernel_size, kernel_size).repeat(c, 1, 1, 1)
    c1, c2 = k1 ** 2, k2 ** 2
    mx, my = F.conv2d(x, k, groups=c), F.conv2d(y, k, groups=c)
    sxx = F.conv2d(x * x, k, groups=c) - mx ** 2
    syy = F.conv2d(y * y, k, groups=c) - my ** 2
    sxy = F.conv2d(x * y, k, groups=c) - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    ss = (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1) * cs
    return ss.mean(dim=(-1, -2)).mean(dim=1).mean()


def _ms_ssim(x, y, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """MS-SSIM with piq.multi_scale_ssim's defaults (5 levels, scale weights 0.0448 ... 0.1333, no initial avg-pool; level k is level
    k-1 replicate-padded by max(H % 2, W % 2) on the top and left, then 2x2 average-pooled).  On the GPU: srk_ms_ssim."""
    if x.is_cuda and kernel_size == 11:
        from .. import ops
        return ops.ms_ssim(x, y, sigma=sigma, k1=k1, k2=k2)
    return _ms_ssim_torch(x, y, kernel_size, sigma, k1, k2)


def _ms_ssim_torch(x, y, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """The plain-torch fp32 form of _ms_ssim (the CPU path; tools/microbench_ms_ssim.py also times it on the GPU)."""
    from ..ops_metrics import MS_SSIM_WEIGHTS, ms_ssim_check
    ms_ssim_check(x, y)
    x, y = x.float(), y.float()
    c = x.shape[1]
    co = torch.arange(kernel_size, dtype=torch.float32, device=x.device) - (kernel_size - 1) / 2.0
    g = torch.exp(-(co ** 2) / (2 * sigma ** 2))
    g = g / g.sum()
    k = torch.outer(g, g).view(1, 1, kernel_size, kernel_size).repeat(c, 1, 1, 1)
    c1, c2 = k1 ** 2, k2 ** 2
    v = 1.0
    for level, wt in enumerate(MS_SSIM_WEIGHTS):
        if level > 0:
            p = max(x.shape[-2] % 2, x.shape[-1] % 2)
            x = F.avg_pool2d(F.pad(x, [p, 0, p, 0], mode="replicate"), 2)
            y = F.avg_pool2d(F.pad(y, [p, 0, p, 0], mode="replicate"), 2)
        # moments of the images shifted by their plane means: the variances lose no digits to cancellation in fp32
        kx, ky = x.mean(dim=(-1, -2), keepdim=True), y.mean(dim=(-1, -2), keepdim=True)
        xs, ys = x - kx, y - ky
        mx, my = F.conv2d(xs, k, groups=c), F.conv2d(ys, k, groups=c)
        sxx = F.conv2d(xs * xs, k, groups=c) - mx ** 2
        syy = F.conv2d(ys * ys, k, groups=c) - my ** 2
        sxy = F.conv2d(xs * ys, k, groups=c) - mx * my
        mx, my = mx + kx, my + ky
        cs = (2 * sxy + c2) / (sxx + syy + c2)
        m = cs if level < len(MS_SSIM_WEIGHTS) - 1 else (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1) * cs
        v = v * torch.relu(m.mean(dim=(-1, -2))) ** wt
    return v.mean(dim=1).mean()


def _psnr_y(x, y, shave):
    """PSNR on BT.601 luma with a `shave`-pixel border removed (the SR community convention)."""
    def lum(t):
        return (65.481 * t[:, 0:1] + 128.553 * t[:, 1:2] + 24.966 * t[:, 2:3] + 16.0) / 255.0
    xl, yl = lum(x.float()), lum(y.float())
    if shave > 0:
        xl, yl = xl[..., shave:-shave, shave:-shave], yl[..., shave:-shave, shave:-shave]
    mse = ((xl - yl) ** 2).flatten(1).mean(dim=1)
    return (10.0 * torch.log10(1.0 / mse.clamp_min(1e-12))).mean()


def _psnr_y_metric(x, y):
    """PSNR-Y (BT.601 luma, border = 4 px): the quantity BASELINE.json names; NOT in the reference's table."""
    if x.is_cuda and x.shape[1] == 3:
        from .. import ops
        return ops.psnr(x, y, luma=True, shave=4, eps=0.0)
    return _psnr_y(x, y, 4)


def _flip_metric(x, y):
    """FLIP (losses/flip.py, srmodel.py:49): mean FLIP error of x against y, no gradient; HIP on the GPU."""
    from .. import flip
    return flip.flip(x, y)


def _gmsd_metric(x, y):
    """GMSD (piq.GMSDLoss's value): the deviation of x against y, no gradient, lower is better; HIP forward launches on the GPU."""
    from .. import gmsd
    return gmsd.gmsd(x, y)


_supported_metrics = {"PSNR": _psnr, "SSIM": _ssim, "PSNR-Y": _psnr_y_metric, "FLIP": _flip_metric,   # srmodel.py:47-54 (+ PSNR-Y)
                      "MS-SSIM": _ms_ssim, "GMSD": _gmsd_metric}


def _dtype_from_precision(precision):
    p = str(precision).lower()
    if p.startswith("bf16"):
        return torch.bfloat16
    if p.startswith("16"):
        return torch.float16
    if p.startswith("32"):
        return torch.float32
    raise ValueError(f"precision {precision!r} not understood (32, 16, 'bf16')")


class SRModel(_Base):
    """Base module for super-resolution models (reference: models/srmodel.py:67-143)."""

    def __init__(self,
                 batch_size: int = 16,
                 channels: int = 3,
                 default_root_dir: str = '.',
                 devices: None | list[int] | str | int = None,
                 eval_datasets: list[str] = ['DIV2K', 'Set5', 'Set14', 'B100', 'Urban100'],
                 log_loss_every_n_epochs: int = 5,
                 log_weights_every_n_epochs: int = 50,
                 losses: str = 'l1',
                 max_epochs: int = -1,
                 metrics: list[str] = ['PSNR', 'SSIM'],
                 metrics_for_pbar: list[str] = ['PSNR', 'SSIM'],
                 model_gpus: list[str] = [],
                 model_parallel: bool = False,
                 optimizer: str = 'ADAM',
                 optimizer_params: list[str] = [],
                 patch_size: int = 128,
                 precision: int | str = 32,
                 predict_datasets: list[str] = [],
                 save_results: int = -1,
                 save_results_from_epoch: str = 'last',
                 scale_factor: int = 4,
                 tile: int = 0,
                 tile_pad: int = _tiling.DEFAULT_TILE_PAD,
                 tile_batch: int = _tiling.DEFAULT_TILE_BATCH,
                 self_ensemble: bool = False,
                 ema_decay: float = 0.0,
                 lr_schedule: str = '',
                 lr_schedule_params: list[str] = [],
                 gradient_clip_val: int | float | None = None,
                 gradient_clip_algorithm: str | None = None,
                 accumulate_grad_batches: int = 1,
                 loss_params: list[str] = [],
                 **kwargs: dict[str, Any]):
        super().__init__()
        self._logger = logging.getLogger(__name__)
        self.save_hyperparameters()
        # srmodel.py:105-108
        self.example_input_array = torch.zeros(batch_size, channels, patch_size // scale_factor, patch_size // scale_factor)
        if model_parallel:
            self._logger.warning("model_parallel is vestigial in the reference (SURVEY.md) and ignored here")
        self._model_parallel = False
        self._model_gpus = None
        self._batch_size = batch_size
        self._channels = channels
        self._default_root_dir = default_root_dir
        self._eval_datasets = eval_datasets
        self._last_epoch = max_epochs
        self._log_loss_every_n_epochs = log_loss_every_n_epochs
        self._log_weights_every_n_epochs = log_weights_every_n_epochs
        self._losses = self._create_losses(losses, patch_size, precision, loss_params, channels=channels)
        self._metrics = self._create_metrics(metrics)
        if channels != 3 and ("flip" in {l.name for l in self._losses} or "FLIP" in {m for m, _ in self._metrics}):
            raise ValueError(f"the FLIP loss / metric compares colours and needs channels == 3 (got channels={channels})")
        self._metrics_for_pbar = metrics_for_pbar
        self._optim, self._optim_params = self._parse_optimizer_config(optimizer, optimizer_params)
        self._predict_datasets = predict_datasets
        self._save_results = save_results
        self._save_results_from_epoch = save_results_from_epoch
        self._scale_factor = scale_factor
        self._training_step_outputs = []
        self._validation_step_outputs = []
        #: tiled / x8 self-ensemble evaluation (tiling.py): `tile` is the LR tile side (0: off), `tile_pad` the LR pixels of context a
        #: tile carries beyond what it owns, `tile_batch` how many tiles one forward takes; both off is the whole-image path
        _tiling.check_args(tile, tile_pad, tile_batch)
        self._tile, self._tile_pad, self._tile_batch, self._self_ensemble = tile, tile_pad, tile_batch, bool(self_ensemble)
        #: decay of the exponential moving average of the weights (ema.ParamEMA); 0: off, nothing is allocated and `ema` stays None.
        #: `Trainer.fit` creates the average and updates it behind every optimizer step; `ema_weights()` evaluates under it
        _ema.ParamEMA._check_decay(ema_decay)
        self.ema_decay = float(ema_decay)
        #: learning-rate schedule (lr_sched.DeviceLRSchedule): its kind ('' : none, nothing is built or allocated) and its constants as
        #: `name=value` strings, e.g. "cosine", ["t_max=300000", "eta_min=1e-7", "warmup_steps=2000"]; checked here, built by
        #: `configure_optimizers()` and attached to the optimizer it returns (`optimizer.lr_schedule`)
        self._lr_schedule = str(lr_schedule)
        if self._lr_schedule:
            self._lr_schedule_constants = _lr_sched.parse_params(self._lr_schedule, list(lr_schedule_params))
        elif lr_schedule_params:
            raise ValueError(f"lr_schedule_params {list(lr_schedule_params)} without an lr_schedule")
        #: gradient clipping (grad_clip.GradClip), under Lightning's Trainer keys and defaults: `gradient_clip_val` None is off (nothing
        #: is built or allocated), `gradient_clip_algorithm` None means "norm"; checked here, built by `configure_optimizers()` and
        #: attached to the optimizer it returns (`optimizer._clip`)
        self._clip_algorithm = "norm" if gradient_clip_algorithm is None else gradient_clip_algorithm
        self._clip_val = None
        if gradient_clip_val is not None:
            self._clip_val, _ = _grad_clip.check_args(gradient_clip_val, self._clip_algorithm)
        elif self._clip_algorithm not in _grad_clip.ALGORITHMS:
            raise ValueError(f"gradient_clip_algorithm not recognized: {gradient_clip_algorithm!r}. Supported: {', '.join(_grad_clip.ALGORITHMS)}")
        #: gradient accumulation (grad_accum.GradAccum), Lightning's Trainer key: the optimizer steps once per window of this many batches, on
        #: the mean of their gradients; 1 is off (nothing is built or allocated).  Checked here, built by `configure_optimizers()` and
        #: attached to the optimizer it returns (`optimizer._accum`)
        self._accumulate_grad_batches = _grad_accum.check_args(accumulate_grad_batches)
        #: arithmetic type of the HIP path: storage dtype of activations / packed weights (fp32 accumulate)
        self.compute_dtype = _dtype_from_precision(precision)
        #: storage dtype of the validation / predict forward.  bf16 keeps 8 mantissa bits on the residual trunk, which
        #: costs 0.005-0.013 dB of PSNR on a trained EDSR-baseline (tests/test_gpu_fullsize_parity.py); fp16 storage runs at the same
        #: speed and stays within 0.0002 dB of the fp32 reference path, so a bf16 model evaluates in fp16 unless told
        #: otherwise (`eval_precision=` 32 / 16 / 'bf16'; non-finite fp16 outputs fall back to the training dtype)
        ep = kwargs.get("eval_precision")
        self.eval_dtype = _dtype_from_precision(ep) if ep is not None else \
            (torch.float16 if self.compute_dtype == torch.bfloat16 else self.compute_dtype)

    #: the `ema.ParamEMA` of the parameters once `make_ema()` has run.  Not a module buffer: `state_dict()` keeps the reference's layout
    ema = None

    def make_ema(self, decay=None):
        """Create the average of every floating-point parameter (`decay`: `ema_decay` unless given).  Its shadows start from the
        current weights and its device table names their addresses, so call it once the model is on its device and any checkpoint is
        loaded."""
        self.ema = _ema.ParamEMA(self.parameters(), self.ema_decay if decay is None else decay)
        return self.ema

    def ema_weights(self):
        """Context manager: the model runs on the averaged weights inside the block (`ParamEMA.swapped`: exchanged in place, the live
        ones are back afterwards); a null context when there is no average.  With a `GraphedStep` that still has an update pending,
        `flush()` first."""
        return self.ema.swapped() if self.ema is not None else contextlib.nullcontext()

    #: a `DeviceLRSchedule.state_dict()` (a checkpoint's) that the next `configure_optimizers()` loads into the schedule it builds
    lr_schedule_state = None
    #: a `GradClip.state_dict()` (a checkpoint's) that the next `configure_optimizers()` loads into the clipper it builds
    grad_clip_state = None

    # -- optimizers: srmodel.py:145-154 ------------------------------------------------------------
    def configure_optimizers(self):
        """`[optimizer]`, as the reference returns it; with `lr_schedule` the schedule is attached to it (`optimizer.lr_schedule`: it
        advances behind every `optimizer.step()` by itself), with `gradient_clip_val` the clipper (`optimizer._clip`: its launches run inside
        `optimizer.step()`), with `accumulate_grad_batches` > 1 the accumulator (`optimizer._accum`: callers step through its `step()`).  Call it
        once the model is on its device."""
        trainable = filter(lambda p: p.requires_grad, itertools.chain(self.parameters()))
        optimizer = self._optim(trainable, **self._optim_params)
        if self._lr_schedule:
            sched = _lr_sched.DeviceLRSchedule(optimizer, self._lr_schedule, **self._lr_schedule_constants)
            if self.lr_schedule_state is not None:
                sched.load_state_dict(self.lr_schedule_state)
        if self._clip_val is not None:
            clip = _grad_clip.GradClip(optimizer, self._clip_val, self._clip_algorithm)
            if self.grad_clip_state is not None:
                clip.load_state_dict(self.grad_clip_state)
        if self._accumulate_grad_batches > 1:
            _grad_accum.GradAccum(optimizer, self._accumulate_grad_batches)
        return [optimizer]

    def forward(self, x):  # srmodel.py:156-158 (abstract)
        raise NotImplementedError

    def _pack_group(self):
        """Lazily created `ops.PackGroup` of the CURRENT storage dtype: one launch per step re-packs every conv's shadow
        weights.  One group per dtype, so the fp16 evaluation forward of a bf16 model (`_eval_forward`) never adds its
        entries to the group the (possibly hipGraph-captured) training step refreshes."""
        groups = self.__dict__.get("_srk_packs")
        if groups is None:
            groups = self.__dict__["_srk_packs"] = {}
        g = groups.get(self.compute_dtype)
        if g is None:
            from .. import ops
            g = groups[self.compute_dtype] = ops.PackGroup()
        return g

    # -- srmodel.py:160-171 ---------------------------------------------------------------------------
    def training_step(self, batch, batch_idx):
        img_sr = self.forward(batch['lr'])
        result = self._calculate_losses(img_sr=img_sr, img_hr=batch['hr'])
        return result

    def _eval_forward(self, x):
        """`forward` in the evaluation storage dtype (see `eval_dtype`)."""
        if self._tile or self._self_ensemble:
            return self._eval_forward_tiled(x)
        if self.eval_dtype == self.compute_dtype or not x.is_cuda:
            return self.forward(x)
        prev, self.compute_dtype = self.compute_dtype, self.eval_dtype
        try:
            y = self.forward(x)
        finally:
            self.compute_dtype = prev
        if self.eval_dtype == torch.float16 and not bool(torch.isfinite(y).all()):
            y = self.forward(x)                   # fp16 range exceeded: the training dtype's answer
        return y

    def _eval_forward_tiled(self, x):
        """`_eval_forward` through tiling.tiled_forward: the same dtype rule, applied to the assembled image (one sync)."""
        def run():
            return _tiling.tiled_forward(self.forward, x, self._scale_factor, tile=self._tile, pad=self._tile_pad,
                                         tile_batch=self._tile_batch, self_ensemble=self._self_ensemble)
        if self.eval_dtype == self.compute_dtype or not x.is_cuda:
            return run()
        prev, self.compute_dtype = self.compute_dtype, self.eval_dtype
        try:
            y = run()
        finally:
            self.compute_dtype = prev
        if self.eval_dtype == torch.float16 and not bool(torch.isfinite(y).all()):
            y = run()                             # fp16 range exceeded: the training dtype's answer
        return y

    # -- srmodel.py:214-232 (metric core; image dumping is out of scope) ----------------------------
    def validation_step(self, batch, batch_idx, dataloader_idx=0):
        img_lr, img_hr = batch['lr'], batch['hr']
        img_sr = self._eval_forward(img_lr)
        assert img_sr.size() == img_hr.size(), \
            f'Output size for image {self._eval_datasets[dataloader_idx]}/{batch.get("path")} should be {img_hr.size()}, instead is {img_sr.size()}'
        img_hr = img_hr.clamp(0, 1)
        img_sr = img_sr.clamp(0, 1)
        result = self._calculate_metrics(img_sr=img_sr, img_hr=img_hr, dataloader_idx=dataloader_idx)
        self._validation_step_outputs.append(result)
        return result

    # -- srmodel.py:345-373 ---------------------------------------------------------------------------
    def on_validation_epoch_end(self):
        """Plain mean of the per-image metrics, per key (`<dataset>/<metric>`): what the reference logs at the end of a
        validation epoch.  The result is also kept in `last_validation_metrics` (no Lightning logger needed) and the
        step outputs are cleared (they hold device tensors)."""
        trainer = getattr(self, "_trainer", None)
        if not self._validation_step_outputs or (trainer is not None and getattr(trainer, "sanity_checking", False)):
            self._validation_step_outputs.clear()
            return {}

        def _mean(keys, metrics):
            out = {}
            for k in keys:
                vals = [m[k] for m in metrics if k in m]
                out[k] = torch.stack([torch.as_tensor(v).squeeze().float() for v in vals]).mean().cpu().detach()
            return out

        outs = self._validation_step_outputs
        metrics_dict = {}
        if isinstance(outs[0], dict):                       # one list of per-batch dicts (keys carry the dataset name)
            keys = []
            for m in outs:
                keys += [k for k in m if k not in keys]
            metrics_dict.update(_mean(keys, outs))
        else:                                               # list (per dataset) of lists of dicts
            for dataset_result in outs:
                metrics_dict.update(_mean(dataset_result[0].keys(), dataset_result))
        self.log_dict(metrics_dict, prog_bar=False, logger=True, add_dataloader_idx=False)
        self.last_validation_metrics = metrics_dict
        self._validation_step_outputs.clear()
        return metrics_dict

    # -- srmodel.py:375-433: forward + clamp + PNG on disk (the logger image dumps are out of scope) -------------
    def predict_step(self, batch, batch_idx, dataloader_idx=0):
        img_sr = self._eval_forward(batch['lr']).clamp(0, 1)
        if self._predict_datasets and 'path' in batch and dataloader_idx < len(self._predict_datasets):
            from pathlib import Path
            local = Path(f'{self._default_root_dir}') / self._predict_datasets[dataloader_idx]
            local.mkdir(parents=True, exist_ok=True)
            name = batch['path'][0]
            self.save_png(img_sr[0], local / f'{name}.png')
            h, w = img_sr.shape[-2:]
            if h >= 96 and w >= 96:                          # K.CenterCrop(96) of the reference (srmodel.py:382-392)
                t, l = (h - 96) // 2, (w - 96) // 2
                self.save_png(img_sr[0, :, t:t + 96, l:l + 96], local / f'{name}_center.png')
        return img_sr

    @staticmethod
    def to_uint8(img):
        """torchvision.utils.save_image rounding (srmodel.py:311-315): floor(clamp(x,0,1)*255 + 0.5)."""
        return torch.floor(img.clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)

    @classmethod
    def save_png(cls, img, path):
        """One CHW float image -> PNG with torchvision.utils.save_image's rounding (srmodel.py:409-412), through PIL."""
        from PIL import Image
        u8 = cls.to_uint8(img.detach().float()).permute(1, 2, 0).cpu().numpy()
        Image.fromarray(u8[..., 0] if u8.shape[2] == 1 else u8).save(str(path))

    # the packed-weight group holds ctypes tables with device pointers: never copied / pickled with the module
    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_srk_packs", None)
        state.pop("_srk_wn", None)
        state.pop("ema", None)               # (device table, page-locked staging buffer; a copy of the module starts without an average)
        return state

    # -- srmodel.py:435-501 ------------------------------------------------------------------------------
    def _create_losses(self, losses_str: str, patch_size: int, precision=32, loss_params=(), channels=3) -> list[_SubLoss]:
        """`loss_params`: the pixel losses' parameters as `<loss>.<key>=<value>` strings (pixel_loss.pixel_loss_parse_params), e.g.
        ["charbonnier.eps=1e-6", "robust.alpha=-2", "robust.c=0.05"], the focal frequency loss's `ffl.alpha=...`
        (freq_loss.freq_loss_parse_params) and the VGG loss's `vgg.weights=...`, `vgg.layer=...`, ... (vgg_loss.vgg_loss_parse_params);
        an entry must name a loss of `losses_str`."""
        losses = []
        for loss in losses_str.split('+'):
            loss_split = loss.split('*')
            if len(loss_split) == 2:
                weight, loss_type = loss_split
                try:
                    weight = float(weight)
                except ValueError:
                    raise ValueError(f'{weight} is not a valid number to be used as weight for loss function {loss_type.strip()}')
            else:
                weight = 1.
                loss_type = loss_split[0]
            loss_type = loss_type.strip().lower()
            if loss_type in _supported_losses:
                fn = _supported_losses[loss_type]
            elif loss_type in _out_of_scope_losses:
                raise NotImplementedError(f'loss {loss_type} needs piq/kornia/robust_loss_pytorch and is outside this build '
                                          f'(SURVEY.md section 2 row 12). Supported: {", ".join(_supported_losses)}')
            else:
                raise AttributeError(f'Couldn\'t find loss {loss_type}. Supported losses: {", ".join(_supported_losses)}')
            if loss_type == "ms_ssim" and patch_size < _MS_SSIM_MIN_PATCH:
                raise ValueError(f'loss ms_ssim needs an HR patch of at least {_MS_SSIM_MIN_PATCH} (five levels of an 11-tap filter), '
                                 f'got patch_size={patch_size}')
            losses.append(_SubLoss(name=loss_type, loss=fn, weight=weight))
        names = [l.name for l in losses]
        if "vgg" in names and channels != 3:
            raise ValueError(f"the VGG loss compares RGB images and needs channels == 3 (got channels={channels})")
        if loss_params or any(name in _pixel_losses or name in ("ffl", "vgg") for name in names):
            from ..freq_loss import freq_loss_parse_params
            from ..pixel_loss import pixel_loss_parse_params
            # ffl's entries are its own (its alpha obeys another rule than robust's), and so are vgg's (a path, names); every other entry,
            # `fft.x=...` and an `ffl....` or `vgg....` without the loss among them, is refused where it always was

            def entries_of(name):
                return [e for e in loss_params if name in names and str(e).strip().lower().partition(".")[0].strip() == name]
            own, own_vgg = entries_of("ffl"), entries_of("vgg")
            params = pixel_loss_parse_params(names, [e for e in loss_params if e not in own and e not in own_vgg])
            if "ffl" in names:
                params.update(freq_loss_parse_params(own))
            for l in losses:
                if l.name in params:
                    l.loss = functools.partial(l.loss, **params[l.name])
            if "vgg" in names:
                from .. import vgg_loss
                # one callable that owns the frozen weights, shared by every `vgg` term of the string; NOT a submodule: state_dict(),
                # parameters() and with them the optimizers, the EMA, clipping and DDP never see it
                vp = vgg_loss.vgg_loss_parse_params(own_vgg, _dtype_from_precision(precision))
                pools = vgg_loss.vgg_pools(vp["net"], vp["layer"])
                if patch_size < 2 ** pools:
                    raise ValueError(f'loss vgg at {vp["net"]} {vp["layer"]} needs an HR patch of at least {2 ** pools} '
                                     f'({pools} max-pools), got patch_size={patch_size}')
                term = vgg_loss.VGGLoss(**vp)
                for l in losses:
                    if l.name == "vgg":
                        l.loss = term
        return losses

    def _create_metrics(self, metrics: list[str]):
        used = []
        for metric in metrics:
            if metric in _supported_metrics:
                used.append((metric, _supported_metrics[metric]))
            elif metric in {'BRISQUE', 'LPIPS'}:
                raise NotImplementedError(f'metric {metric} needs piq and is outside this build. Supported: {", ".join(_supported_metrics)}')
            else:
                raise AttributeError(f'Couldn\'t find metric {metric}. Supported metrics: {", ".join(_supported_metrics)}')
        return used

    # -- srmodel.py:519-565 ------------------------------------------------------------------------------
    def _calculate_losses(self, img_sr: torch.Tensor, img_hr: torch.Tensor) -> dict[str, torch.Tensor]:
        # same values as the reference's `weight * loss` terms and their `sum()` (srmodel.py:519-565), without the launches a
        # multiplication by 1 and `0 + x` cost (two of the ~8 parameter-sized torch kernels of a batch-16 step)
        losses, names = [], []
        for l in self._losses:
            v = l.loss(img_sr, img_hr)
            losses.append(v if l.weight == 1 else l.weight * v)
            names.append(l.name)
        losses_dict = {f'loss/{k}': v for k, v in zip(names, losses)}
        total = losses[0]
        for v in losses[1:]:
            total = total + v
        losses_dict['loss'] = total
        return losses_dict

    # -- srmodel.py:567-593 ------------------------------------------------------------------------------
    def _calculate_metrics(self, img_sr, img_hr, dataloader_idx: int = 0):
        out = {}
        for name, metric in self._metrics:
            out[f'{self._eval_datasets[dataloader_idx]}/{name}'] = metric(img_sr, img_hr)
        return out

    # -- srmodel.py:595-621 ------------------------------------------------------------------------------
    def _parse_optimizer_config(self, optimizer: str, optimizer_params: list[str]):
        if optimizer in _supported_optimizers:
            optimizer_class = _supported_optimizers[optimizer]
        elif optimizer in _out_of_scope_optimizers:
            raise NotImplementedError(f'optimizer {optimizer} needs torch_optimizer and is outside this build')
        else:
            raise ValueError(f'Optimizer not recognized: {optimizer}. Supported optimizers: {", ".join(_supported_optimizers)}')
        # The reference re-binds `optimizer_params = {}` BEFORE iterating it (srmodel.py:602-603), so every
        # user-supplied entry is dropped and the optimizer runs at torch defaults.  Kept for parity
        # (pinned by tests/golden/traj_*): the argument is accepted and has no effect.
        return optimizer_class, {}
