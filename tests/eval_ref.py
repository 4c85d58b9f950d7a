"""Shared helpers of the whole-image evaluation tests (test_gpu_eval_images.py, test_eval_ref_cpu.py, and
test_full_image_inference_vs_oracle in test_gpu_models.py) -- TEST INFRASTRUCTURE, never imported by the product.

One implementation of "compare a whole image at batch 1 with the oracle":

* the reference is `oracle.functional.forward` in float64 on the model's own default initialisation under
  `torch.manual_seed(0)` (SRResNet: plus seeded, non-trivial BatchNorm running statistics), copied before `.cuda()`;
* the input is a smooth pattern plus noise in [0,1] (`image`), as test_ssim_device_reduction builds one;
* per case the oracle runs once clean and once per storage dtype with every floating tensor of the state dict and the
  input rounded to that dtype and back (`RefCache`) -- except the frozen MeanShift constants (sub_mean / add_mean), which the
  build adds as fp32 vectors inside its head and tail kernels and never stores in 16 bits (WDSR's mean is a constant of the
  oracle's code and is not rounded either): rounding add_mean shifts every pixel of a channel by the same amount, which
  is no position effect and pulls the peak / RMS baseline below what ANY noise-like error has (measured: 1.2-1.4 for D-DBPN,
  2.3-3.3 for EDSR, against 4.5-5 for Gaussian noise over this many pixels).  The difference of those two runs is what rounding the OPERANDS alone
  does to the image; its statistics (`local_stats`) are the baseline of the position checks, and the limit is
  baseline x MARGIN (the build also rounds the activations of every layer, which the weight-rounded oracle does not).

Position checks (PSNR averages a wrong tile edge away): from e = y - ref minus its per-channel mean
  row  = max / median of the per-row RMS of e (over columns and channels)
  col  = max / median of the per-column RMS of e
  peak = max|e| / RMS(e)

The per-channel mean is removed because a constant has no position.  Rounding the bias of a net's LAST convolution moves every
pixel of a channel by the same amount, and where the default-initialised image is small that constant IS the baseline: in the
operands-rounded oracle runs of D-DBPN it carries 48 % (x4), 79-85 % (x2) and 98-99 % (x8) of the error's energy, against 3-9 % for
EDSR and RDN, and holds the baseline peak / RMS at 1.7-3.7 -- below the 4.2-4.9 that the largest of this many Gaussian samples
reaches, so twice that baseline is a limit no noise-like error can meet, whatever produced it (the build, which adds the bias in
fp32, has no such constant).  With the mean removed D-DBPN's baselines are 3.7-4.9 (table).  A constant in
the BUILD's error only lowers these ratios, so removing it makes the checks stricter on the build; the offset itself is held by
the fp32 bound, the PSNR floors and the PSNR-against-HR criterion.

PSNR floors are the project's (test_random_input_16bit_vs_oracle): 50 dB for bf16 storage, 62 dB for fp16; a bf16 model's
`predict_step` evaluates in fp16 (`SRModel.eval_dtype`) and is judged at the fp16 floor.  Where the weight-rounded oracle run
itself comes within FLOOR_MARGIN_DB of a floor, the floor of that case is that run's PSNR - FLOOR_MARGIN_DB (6 dB: the same
factor 2, in RMS, as MARGIN): rounding the operands alone already costs that much, the cause is in the network, not in a
kernel.  With the cases below that rule lowers no floor (the closest is WDSR in bf16, see the table; test_eval_ref_cpu.py
asserts it), so every case is judged at 50 / 62 dB.

The uint8 contract (|to_uint8(y) - to_uint8(ref)| <= 1, share of differing pixels < 1e-3 fp32 / < 0.08 fp16) is what
`predict_step` promises, so it is asserted for fp32 and fp16 evaluation.  bf16 STORAGE (eval_precision='bf16') at its 50 dB
floor has an RMS error of 0.8 / 255: neither half of the contract can be demanded of the format, and it is not asserted there.

fp32 storage: the parameters and the image are fp32 already, so the operands-rounded run IS the clean run; its position
statistics are judged by the fp16 baseline's (ratios: the shape of a rounding error, not its size).

Baselines measured on the CPU (float64 oracle, operands rounded to the dtype vs clean; `python tests/eval_ref.py` prints
this table; test_eval_ref_cpu.py asserts row, col < 3 and the uint8 caps, the GPU test recomputes every number):

  case                      dtype    row    col    peak   PSNR dB  u8 share
  ------------------------  -----  -----  -----  ------  -------  --------
  edsr_x4_85x123            fp16    1.17   1.12    5.15    93.40  4.3e-03
  edsr_x4_85x123            bf16    1.17   1.17    5.73    75.64  3.3e-02
  edsr_x4_308x322           fp16    1.13   1.19    6.28    93.67  4.1e-03
  edsr_x4_308x322           bf16    1.27   1.13    6.26    76.18  3.1e-02
  edsr_x4_309x322           fp16    1.14   1.19    6.49    93.67  4.2e-03
  edsr_x4_309x322           bf16    1.26   1.15    6.13    76.18  3.1e-02
  edsr_x4_339x510           fp16    1.18   1.12    5.92    93.32  4.4e-03
  edsr_x4_339x510           bf16    1.16   1.15    6.40    75.56  3.4e-02
  edsr_x4_61x256            fp16    1.14   1.23    5.85    93.77  4.4e-03
  edsr_x4_61x256            bf16    1.26   1.15    5.75    76.26  3.1e-02
  edsr_x4_61x257            fp16    1.12   1.22    5.98    93.76  4.2e-03
  edsr_x4_61x257            bf16    1.24   1.23    5.33    76.27  3.1e-02
  edsr_x2_37x512            fp16    1.16   1.25    4.47    89.89  6.6e-03
  edsr_x2_37x512            bf16    1.17   1.18    5.74    72.74  4.6e-02
  edsr_x2_37x513            fp16    1.14   1.25    4.89    89.91  6.6e-03
  edsr_x2_37x513            bf16    1.11   1.21    5.32    72.76  4.6e-02
  edsr_x3_47x173            fp16    1.18   1.15    4.48    89.55  6.7e-03
  edsr_x3_47x173            bf16    1.12   1.17    5.59    71.50  5.3e-02
  edsr_gray_x4_61x45        fp16    2.63   1.95    5.31    88.84  5.8e-03
  edsr_gray_x4_61x45        bf16    1.62   1.35    4.87    70.48  4.8e-02
  edsr_large_x2_141x150     fp16    1.15   1.12    4.90    90.97  5.5e-03
  edsr_large_x2_141x150     bf16    1.13   1.20    4.83    72.77  4.5e-02
  rcan_48x48                fp16    1.43   1.24    5.59    92.90  4.4e-03
  rcan_48x48                bf16    1.15   1.10    5.01    74.34  3.9e-02
  rcan_112x112              fp16    1.36   1.19    5.55    92.65  4.5e-03
  rcan_112x112              bf16    1.17   1.11    5.30    74.28  3.9e-02
  rcan_113x112              fp16    1.37   1.21    5.81    92.65  4.8e-03
  rcan_113x112              bf16    1.16   1.12    5.21    74.26  3.9e-02
  rcan_248x264              fp16    1.36   1.21    6.08    92.59  4.7e-03
  rcan_248x264              bf16    1.15   1.09    5.39    74.20  3.9e-02
  rcan_256x256              fp16    1.38   1.20    6.03    92.58  4.6e-03
  rcan_256x256              bf16    1.15   1.09    5.62    74.20  3.9e-02
  rcan_256x257              fp16    1.37   1.20    6.43    92.58  4.7e-03
  rcan_256x257              bf16    1.15   1.08    5.85    74.20  3.9e-02
  rcan_309x322              fp16    1.37   1.22    6.16    92.58  4.6e-03
  rcan_309x322              bf16    1.15   1.09    5.49    74.20  3.9e-02
  rcan_339x510              fp16    1.36   1.20    6.93    92.56  4.7e-03
  rcan_339x510              bf16    1.14   1.09    5.78    74.19  3.9e-02
  rdn_a_x4_75x101           fp16    1.19   1.35    7.64    94.85  2.2e-03
  rdn_a_x4_75x101           bf16    1.18   1.93    6.89    75.24  2.1e-02
  rdn_b_x4_45x59            fp16    1.93   1.67    5.78    91.57  3.6e-03
  rdn_b_x4_45x59            bf16    1.57   1.18    5.16    75.20  2.5e-02
  wdsr_a_x4_45x59           fp16    1.22   1.15    5.42    78.84  2.3e-02
  wdsr_a_x4_45x59           bf16    1.18   1.16    5.23    60.72  1.8e-01
  wdsr_b_x4_85x123          fp16    1.07   1.16    5.50    80.56  1.9e-02
  wdsr_b_x4_85x123          bf16    1.30   1.09    5.32    61.87  1.6e-01
  wdsr_b_x4_339x510         fp16    1.15   1.14    6.01    80.98  1.8e-02
  wdsr_b_x4_339x510         bf16    1.23   1.08    6.23    62.98  1.4e-01
  srresnet_x4_75x101        fp16    1.27   1.43    4.44    90.86  4.7e-03
  srresnet_x4_75x101        bf16    1.61   1.83    5.29    73.85  3.1e-02
  srresnet_x2_53x71         fp16    1.41   1.30    5.26    90.96  3.6e-03
  srresnet_x2_53x71         bf16    1.49   1.33    5.06    73.53  2.9e-02
  srresnet_x3_41x67         fp16    1.48   2.53    6.91    90.73  3.3e-03
  srresnet_x3_41x67         bf16    1.39   1.66    5.58    73.83  2.7e-02
  ddbpn_x2_61x45            fp16    2.08   1.29    4.23   107.07  1.0e-03
  ddbpn_x2_61x45            bf16    1.17   1.24    3.65    85.92  1.0e-02
  ddbpn_x4_45x59            fp16    1.41   1.94    4.66   113.07  3.2e-04
  ddbpn_x4_45x59            bf16    1.14   1.63    4.51    95.70  2.8e-03
  ddbpn_x8_29x37            fp16    1.65   1.56    4.90   105.56  1.1e-03
  ddbpn_x8_29x37            bf16    1.90   1.43    4.87    87.71  1.3e-02
"""
import math
import os
import sys
from contextlib import contextmanager
from dataclasses import dataclass, field

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))       # (run as a script: the repository root)
from oracle import functional as OF, metrics as OM  # noqa: E402

MARGIN = 2.0                      # limit of a position statistic = baseline x MARGIN
FLOOR_MARGIN_DB = 6.0             # a floor taken from the weight-rounded oracle run: that run's PSNR minus this
PSNR_FLOOR = {torch.bfloat16: 50.0, torch.float16: 62.0}        # test_random_input_16bit_vs_oracle
FP32_REL = 1e-3                   # `rel` bound of test_gpu_models.py (north_star: conv activations within 1e-3 in fp32)
U8_SHARE = {torch.float32: 1e-3, torch.float16: 0.08}           # test_full_image_inference_vs_oracle
PROFILE_MAX = 3.0                 # a baseline row / column ratio at or above this means a badly chosen input image
# validation_step: HR = clamp(ref) + noise of this PSNR.  28 dB is what x4 models reach on the usual sets, and it is where the floors
# above IMPLY the PSNR criteria of test_gpu_fullsize_parity.py for an error that is uncorrelated with the image: dPSNR = 10 log10(1 +
# mse_e / mse_n) is 0.027 dB at 50 dB (bound 0.03, bf16) and 0.0017 dB at 62 dB (bound 0.01, fp16).  An error that is NOT noise-like
# (a bias, a shifted tile) moves PSNR against HR by more than its own energy and is what this check adds to the floors.
HR_PSNR_DB = 28.0
DPSNR = {torch.float32: 0.01, torch.float16: 0.01, torch.bfloat16: 0.03}
PREC = {torch.float32: 32, torch.float16: 16, torch.bfloat16: "bf16"}
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@dataclass(frozen=True)
class Case:
    """One (model, LR size).  `expect` names the side of each routing threshold the size is on; the GPU test asserts it through
    the project's own predicates and counters (`assert_routing`):
      pair   : every `ops.pair_ok` call of a 16-bit run says this (the one-launch 3x3 pair vs weight-stationary / conv_ks)
      hr     : the `ops.hr_tail_ok` call of a 16-bit run says this (collapsed 5x5 HR stage)
      lazy   : 16-bit RCAN: srk_conv_pair launches with the previous block's channel attention folded in (ca_mode 2) happen / do not
      splits : `srk_ca_splits(1, H * W)` returns exactly this
      ks_ragged : 256-feature conv_ks launch: more 16x16 tiles x output blocks than CUs, tiles not a multiple of the slots"""
    id: str
    cls: str
    kw: dict
    h: int
    w: int
    val: bool = False             # also through validation_step
    expect: dict = field(default_factory=dict)

    @property
    def scale(self):
        return self.kw.get("scale_factor", 4)

    @property
    def channels(self):
        return self.kw.get("channels", 3)


_EDSR = dict(n_feats=64, n_resblocks=16, res_scale=0.1, scale_factor=4)              # EDSR-baseline (tests/golden/manifest.json)
_EDSR4 = dict(n_feats=64, n_resblocks=4, res_scale=0.1)                              # EDSR-baseline's width, depth cut for oracle time
_RCAN = dict(n_feats=64, n_resgroups=2, n_resblocks=3, reduction=16, scale_factor=4)

# Sizes come from the routing code (ops.pair_ok: N * ceil(H/14) * ceil(W/14) tiles against 2 x CUs = 512; ops.hr_tail_ok: max(h, w) <= 512
# at the last stage's input; ops.rcab_chain: <= 64 tiles for the lazy channel attention; ca.hip split_for: min(1024, ceil(HW / 64)) blocks
# of ceil(HW / that) pixels).  srk_ca_splits(1, HW) changes every 64 pixels below HW = 65536 -- about a thousand times between 48x48 and
# 339x510 -- so the cases take both sides of its two REGIME changes instead: the cap (1023 -> 1024 blocks of 64 pixels) and the first size
# past the cap, where blocks grow to 65 pixels, the count DROPS (1013) and the last block is ragged; plus the two ends of the range.
CASES = [
    Case("edsr_x4_85x123", "EDSR", _EDSR, 85, 123, val=True, expect=dict(pair=True, hr=True)),                      # 63 tiles; HR stage input 170x246
    Case("edsr_x4_308x322", "EDSR", dict(_EDSR4, scale_factor=4), 308, 322, expect=dict(pair=True, hr=False)),      # 22 x 23 = 506 tiles
    Case("edsr_x4_309x322", "EDSR", dict(_EDSR4, scale_factor=4), 309, 322, expect=dict(pair=False, hr=False)),     # 23 x 23 = 529 tiles
    Case("edsr_x4_339x510", "EDSR", _EDSR, 339, 510, val=True, expect=dict(pair=False, hr=False)),                  # DIV2K x4 LR: 925 tiles
    Case("edsr_x4_61x256", "EDSR", dict(_EDSR4, scale_factor=4), 61, 256, expect=dict(pair=True, hr=True)),         # HR stage input 122 x 512
    Case("edsr_x4_61x257", "EDSR", dict(_EDSR4, scale_factor=4), 61, 257, expect=dict(pair=True, hr=False)),        # HR stage input 122 x 514
    Case("edsr_x2_37x512", "EDSR", dict(_EDSR4, scale_factor=2), 37, 512, val=True, expect=dict(pair=True, hr=True)),
    Case("edsr_x2_37x513", "EDSR", dict(_EDSR4, scale_factor=2), 37, 513, expect=dict(pair=True, hr=False)),
    Case("edsr_x3_47x173", "EDSR", dict(_EDSR4, scale_factor=3), 47, 173, val=True, expect=dict(pair=True, hr=False)),   # PixelShuffle(3): never collapsed
    Case("edsr_gray_x4_61x45", "EDSR", dict(n_feats=64, n_resblocks=4, res_scale=1, scale_factor=4, channels=1), 61, 45, val=True,
         expect=dict(pair=True, hr=True)),
    Case("edsr_large_x2_141x150", "EDSR", dict(n_feats=256, n_resblocks=2, res_scale=0.1, scale_factor=2), 141, 150, val=True,
         expect=dict(hr=False, ks_ragged=True)),                                                        # 9 x 10 = 90 tiles of 16x16, x 4 output blocks
    Case("rcan_48x48", "RCAN", _RCAN, 48, 48, expect=dict(pair=True, lazy=True, hr=True, splits=36)),
    Case("rcan_112x112", "RCAN", _RCAN, 112, 112, expect=dict(pair=True, lazy=True, hr=True, splits=196)),          # 64 tiles
    Case("rcan_113x112", "RCAN", _RCAN, 113, 112, val=True, expect=dict(pair=True, lazy=False, hr=True, splits=198)),   # 72 tiles
    Case("rcan_248x264", "RCAN", _RCAN, 248, 264, expect=dict(pair=True, lazy=False, hr=False, splits=1023)),       # 1023 blocks of 64
    Case("rcan_256x256", "RCAN", _RCAN, 256, 256, expect=dict(pair=True, lazy=False, hr=True, splits=1024)),        # the cap: 1024 blocks of 64
    Case("rcan_256x257", "RCAN", _RCAN, 256, 257, expect=dict(pair=True, lazy=False, hr=False, splits=1013)),       # past it: blocks of 65, last one ragged
    Case("rcan_309x322", "RCAN", _RCAN, 309, 322, expect=dict(pair=False, lazy=False, hr=False, splits=1016)),      # 529 tiles: 16-bit takes srk_ca_pool
    Case("rcan_339x510", "RCAN", _RCAN, 339, 510, val=True, expect=dict(pair=False, lazy=False, hr=False, splits=1024)),   # blocks of 169 pixels
    Case("rdn_a_x4_75x101", "RDN", dict(rdn_config="A", scale_factor=4), 75, 101, val=True),
    Case("rdn_b_x4_45x59", "RDN", dict(rdn_config="B", scale_factor=4), 45, 59, val=True),
    Case("wdsr_a_x4_45x59", "WDSR", dict(type="A", scale_factor=4), 45, 59, val=True),
    Case("wdsr_b_x4_85x123", "WDSR", dict(type="B", scale_factor=4), 85, 123, val=True),
    Case("wdsr_b_x4_339x510", "WDSR", dict(type="B", n_resblocks=4, scale_factor=4), 339, 510),                     # depth cut (16 -> 4) for oracle time
    Case("srresnet_x4_75x101", "SRResNet", dict(scale_factor=4), 75, 101, val=True),
    Case("srresnet_x2_53x71", "SRResNet", dict(n_feats=64, n_resblocks=4, scale_factor=2), 53, 71),
    Case("srresnet_x3_41x67", "SRResNet", dict(n_feats=64, n_resblocks=4, scale_factor=3), 41, 67),
    Case("ddbpn_x2_61x45", "DDBPN", dict(scale_factor=2), 61, 45),
    Case("ddbpn_x4_45x59", "DDBPN", dict(scale_factor=4), 45, 59, val=True),
    Case("ddbpn_x8_29x37", "DDBPN", dict(scale_factor=8), 29, 37),
]
BY_ID = {c.id: c for c in CASES}

# the fp16 -> training dtype fallback of SRModel._eval_forward: a reduced EDSR whose head is scaled UP and whose first upsampler conv is
# scaled DOWN by the same factor.  ReLU and the residual adds are homogeneous, so the image barely changes (only the trunk's biases lose
# weight), but the head's output and the whole trunk sit far beyond fp16's 65504.
OVERFLOW = Case("edsr_x2_overflow_45x59", "EDSR", dict(n_feats=64, n_resblocks=2, res_scale=0.1, scale_factor=2), 45, 59)
OVERFLOW_GAIN = 2.0 ** 18                         # the scaled weights themselves stay inside fp16's range


def image(c, h, w, seed):
    """(1, c, h, w) float32 in [0,1]: a smooth pattern plus noise, seeded."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 6.28, h), torch.linspace(0, 9.42, w), indexing="ij")
    ph = torch.arange(c, dtype=torch.float32).view(1, c, 1, 1) * 0.7
    base = 0.5 + 0.25 * torch.sin(yy[None, None] + ph) * torch.cos(xx[None, None] - ph)
    return (base + 0.2 * (torch.rand(1, c, h, w, generator=g) - 0.5)).clamp(0, 1).contiguous()


def case_seed(case):
    return 1000 + 7 * case.h + case.w


def new_model(A, case, precision=32, **extra):
    """The model on the CPU: default initialisation under seed 0; SRResNet's running statistics moved off their initial 0 / 1 by a seeded
    generator (eval() mode reads them).  `OVERFLOW`: the two layers rescaled."""
    torch.manual_seed(0)
    m = getattr(A, case.cls)(precision=precision, **case.kw, **extra)
    g = torch.Generator().manual_seed(99)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
            mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
    if case is OVERFLOW:
        with torch.no_grad():
            m.head[0].weight.mul_(OVERFLOW_GAIN)
            m.head[0].bias.mul_(OVERFLOW_GAIN)
            m.tail[0][0].weight.div_(OVERFLOW_GAIN)
    return m.eval()


def state_of(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _round(t, dt):
    return t.to(dt).double() if dt is not None else t.double()


def oracle(case, sd, x, dt=None):
    """float64 oracle forward, unclamped; `dt`: every floating tensor of `sd` and the input rounded to `dt` and back first."""
    keep = ("sub_mean.", "add_mean.")                      # see the module docstring: constants the build never stores in 16 bits
    sd64 = {k: (_round(v, None if k.startswith(keep) else dt) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    kw = dict(case.kw, training=False) if case.cls == "SRResNet" else case.kw
    with torch.no_grad():
        return OF.forward(case.cls, sd64, _round(x, dt), **kw)


def psnr_db(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10 * math.log10(1.0 / max(mse, 1e-30))


def to_uint8(img):
    """SRModel.to_uint8 (torchvision.utils.save_image's rounding), restated so that the CPU test needs no model."""
    return torch.floor(img.clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)


def u8_diff(a, b):
    """(largest difference, share of differing pixels) of the two images' uint8 forms."""
    d = (to_uint8(a.float()).int() - to_uint8(b.float()).int()).abs()
    return int(d.max()), float((d > 0).float().mean())


def local_stats(e):
    """(row, col, peak) of an error image (1, C, H, W), its per-channel mean removed first: see the module docstring."""
    e = e.double()
    e = e - e.mean(dim=(0, 2, 3), keepdim=True)
    rows = e.pow(2).mean(dim=(0, 1, 3)).sqrt()
    cols = e.pow(2).mean(dim=(0, 1, 2)).sqrt()
    rms = float(e.pow(2).mean().sqrt())
    tiny = 1e-300
    return (float(rows.max() / rows.median().clamp_min(tiny)), float(cols.max() / cols.median().clamp_min(tiny)),
            float(e.abs().max()) / max(rms, tiny))


class Ref:
    """The oracle runs of one case: `ref` (clean, clamped to [0,1]), `raw_max` (largest |value| before the clamp) and per storage dtype the
    weight-rounded run's statistics against it."""

    def __init__(self, case, sd, x):
        self.case, self.sd, self.x = case, sd, x
        raw = oracle(case, sd, x)
        self.raw_max = float(raw.abs().max())
        self.ref = raw.clamp(0, 1)
        self.base = {}

    def baseline(self, dt):
        """dict(row, col, peak, psnr, u8max, u8share) of the run with operands rounded to `dt` against the clean run."""
        if dt == torch.float32 and dt not in self.base:
            # the parameters and the image ARE fp32: rounding them is the identity and the two runs coincide.  The position statistics
            # are ratios -- what zero padding and the image's structure do to the SHAPE of a rounding error, whatever its size -- so
            # fp32 storage is judged by the fp16 baseline's
            self.base[dt] = dict(self.baseline(torch.float16), psnr=300.0, u8max=0, u8share=0.0)
        if dt not in self.base:
            y = oracle(self.case, self.sd, self.x, dt).clamp(0, 1)
            row, col, peak = local_stats(y - self.ref)
            u8max, u8share = u8_diff(y, self.ref)
            self.base[dt] = dict(row=row, col=col, peak=peak, psnr=psnr_db(y, self.ref), u8max=u8max, u8share=u8share)
        return self.base[dt]

    def floor(self, dt):
        """PSNR floor of 16-bit storage `dt` for this case (module docstring)."""
        return min(PSNR_FLOOR[dt], self.baseline(dt)["psnr"] - FLOOR_MARGIN_DB)

    def hr(self):
        """The HR image of validation_step: the clamped reference plus seeded noise at HR_PSNR_DB, clamped."""
        g = torch.Generator().manual_seed(case_seed(self.case) + 1)
        sigma = 10.0 ** (-HR_PSNR_DB / 20.0)
        return (self.ref + sigma * torch.randn(self.ref.shape, generator=g, dtype=torch.float64)).clamp(0, 1).float()


class RefCache:
    """Each (model, size) reference is computed once and shared by every storage dtype (a module-scoped fixture holds one of these)."""

    def __init__(self, A):
        self.A, self._refs = A, {}

    def get(self, case, x=None):
        if case.id not in self._refs:
            sd = state_of(new_model(self.A, case))
            self._refs[case.id] = Ref(case, sd, image(case.channels, case.h, case.w, case_seed(case)) if x is None else x)
        return self._refs[case.id]

    def drop(self, case):
        self._refs.pop(case.id, None)


def check_image(y, ref, dt, what, floor_dt=None, u8=True):
    """Every assertion on one build output `y` (what predict_step returned) against `ref` (a `Ref`), for storage dtype `dt`.
    `floor_dt`: the dtype whose PSNR floor judges it (a bf16 model's predict_step: fp16).  Prints measured value next to limit."""
    case, r = ref.case, ref.ref
    assert tuple(y.shape) == (1, case.channels, case.h * case.scale, case.w * case.scale), f"{what}: shape {tuple(y.shape)}"
    assert y.dtype == torch.float32, f"{what}: dtype {y.dtype}"
    y = y.detach().cpu()
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite pixels"
    assert float(y.min()) >= 0.0 and float(y.max()) <= 1.0, f"{what}: outside [0,1]"
    e = y.double() - r
    base = ref.baseline(dt)
    row, col, peak = local_stats(e)
    lim = {k: MARGIN * base[k] for k in ("row", "col", "peak")}
    psnr = psnr_db(y, r)
    line = f"EVAL {what}: PSNR {psnr:.2f} dB"
    fails = []
    if dt == torch.float32:
        rel = float(e.abs().max()) / max(1.0, ref.raw_max)
        line += f" | rel {rel:.2e} (< {FP32_REL:.0e})"
        if not rel < FP32_REL:
            fails.append(f"max|y - ref| / max(1, max|ref|) = {rel:.3e}")
    else:
        floor = ref.floor(floor_dt or dt)
        line += f" (floor {floor:.2f}; operands-rounded oracle {base['psnr']:.2f})"
        if not psnr >= floor:
            fails.append(f"PSNR(build, oracle) = {psnr:.2f} dB < {floor:.2f}")
    line += f" | row {row:.3f} (< {lim['row']:.3f}) col {col:.3f} (< {lim['col']:.3f}) peak {peak:.2f} (< {lim['peak']:.2f})"
    for k, v in (("row", row), ("col", col), ("peak", peak)):
        if not v < lim[k]:
            fails.append(f"{k} statistic {v:.3f} >= {lim[k]:.3f} (= {MARGIN} x baseline {base[k]:.3f})")
    if u8 and dt in U8_SHARE:
        dmax, share = u8_diff(y, r)
        line += f" | u8 max {dmax} share {share:.2e} (< {U8_SHARE[dt]:.0e})"
        if not (dmax <= 1 and share < U8_SHARE[dt]):
            fails.append(f"uint8: max difference {dmax}, share of differing pixels {share:.3e}")
    print(line)
    assert not fails, f"{what}: " + "; ".join(fails)
    return dict(psnr=psnr, row=row, col=col, peak=peak)


@contextmanager
def routing(A):
    """Record what the project's own routing predicates answer, and the srk_conv_pair launches, during a forward."""
    ops = A.ops
    rec = dict(pair=[], hr=[], launches=None)
    real_pair, real_hr = ops.pair_ok, ops.hr_tail_ok
    before = list(ops.PAIR_LAUNCHES)

    def pair_ok(*a, **k):
        rec["pair"].append(bool(real_pair(*a, **k)))
        return rec["pair"][-1]

    def hr_tail_ok(*a, **k):
        rec["hr"].append(bool(real_hr(*a, **k)))
        return rec["hr"][-1]

    ops.pair_ok, ops.hr_tail_ok = pair_ok, hr_tail_ok
    try:
        yield rec
    finally:
        ops.pair_ok, ops.hr_tail_ok = real_pair, real_hr
        rec["launches"] = [a - b for a, b in zip(ops.PAIR_LAUNCHES, before)]


def assert_routing(A, case, dt, rec):
    """The size is on the side of each threshold that `case.expect` names (16-bit runs; fp32 takes neither fused path at any size)."""
    ex = case.expect
    lib = A._lib.load()
    what = f"{case.id} {dt}"
    sixteen = dt != torch.float32
    if "pair" in ex:
        want = ex["pair"] and sixteen
        tiles, lim = lib.srk_conv_pair_tiles(1, case.h, case.w), 2 * lib.srk_device_cus()
        assert (tiles <= lim) == ex["pair"], f"{what}: {tiles} pair tiles against {lim}"
        assert rec["pair"] and all(p == want for p in rec["pair"]), f"{what}: ops.pair_ok said {rec['pair']}"
        assert (sum(rec["launches"]) > 0) == want, f"{what}: srk_conv_pair launches {rec['launches']}"
    if "hr" in ex:
        want = ex["hr"] and sixteen
        assert rec["hr"] == [want], f"{what}: ops.hr_tail_ok said {rec['hr']}"
    if "lazy" in ex:
        assert (rec["launches"][2] > 0) == (ex["lazy"] and sixteen), f"{what}: srk_conv_pair launches by ca_mode {rec['launches']}"
    if "splits" in ex:
        got = lib.srk_ca_splits(1, case.h * case.w)
        assert got == ex["splits"], f"{what}: srk_ca_splits(1, {case.h * case.w}) = {got}, the case was chosen for {ex['splits']}"
    if ex.get("ks_ragged"):
        cus, ncob = lib.srk_device_cus(), case.kw["n_feats"] // 64
        tiles = -(-case.h // 16) * -(-case.w // 16)
        assert tiles * ncob > cus and tiles % (cus // ncob) != 0, f"{what}: {tiles} tiles x {ncob} blocks on {cus} CUs"


def predict(m, x):
    with torch.no_grad():
        y = m.predict_step({"lr": x.cuda()}, 0)
    torch.cuda.synchronize()
    return y


def compare_predict(A, ref, dt, eval_precision=None, check_route=True, u8=True):
    """A fresh model of storage dtype `dt` with the reference's weights through predict_step, checked against `ref`.
    eval_precision='bf16' shows real bf16 storage; without it a bf16 model evaluates in fp16 and is judged as fp16."""
    case = ref.case
    extra = {} if eval_precision is None else dict(eval_precision=eval_precision)
    m = new_model(A, case, PREC[dt], **extra)
    m.load_state_dict(ref.sd)
    m = m.cuda().eval()
    with routing(A) as rec:
        y = predict(m, ref.x)
    if check_route:
        assert_routing(A, case, m.eval_dtype, rec)
    tag = f"{case.id} precision={PREC[dt]}" + (f" eval_precision={eval_precision}" if eval_precision else "")
    check_image(y, ref, m.eval_dtype, tag, u8=u8)
    return m, y


def compare_validation(m, ref, y):
    """validation_step on the same image: its PSNR is the oracle's formula on the clamped build output, and moves against the
    float64 reference's PSNR by no more than the parity criterion (DPSNR)."""
    case, dt = ref.case, m.eval_dtype
    hr = ref.hr()
    with torch.no_grad():
        out = m.validation_step({"lr": ref.x.cuda(), "hr": hr.cuda(), "path": ["x"]}, 0, dataloader_idx=1)
    torch.cuda.synchronize()
    m._validation_step_outputs.clear()
    got = float(out["Set5/PSNR"])
    want = float(OM.psnr(y.detach().cpu().clamp(0, 1), hr))
    p_ref = float(OM.psnr(ref.ref, hr))
    d = abs(want - p_ref)
    print(f"EVAL {case.id} {dt} validation_step: Set5/PSNR {got:.5f} dB, oracle formula on the build's image {want:.5f} (|diff| < 1e-4); "
          f"|PSNR(build, HR) - PSNR(ref, HR)| = {d:.5f} dB (< {DPSNR[dt]})")
    assert abs(got - want) < 1e-4, f"{case.id} {dt}: validation_step PSNR {got} vs {want}"
    assert d < DPSNR[dt], f"{case.id} {dt}: |PSNR(build, HR) - PSNR(ref, HR)| = {d:.5f} dB"


def baseline_table(A, cases=CASES):
    """The docstring's table, computed (CPU)."""
    lines = ["  case                      dtype    row    col    peak   PSNR dB  u8 share",
             "  ------------------------  -----  -----  -----  ------  -------  --------"]
    cache = RefCache(A)
    for c in cases:
        r = cache.get(c)
        for dt, nm in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
            b = r.baseline(dt)
            lines.append(f"  {c.id:<24}  {nm:<5}  {b['row']:5.2f}  {b['col']:5.2f}  {b['peak']:6.2f}  {b['psnr']:7.2f}  {b['u8share']:.1e}")
        cache.drop(c)
    return "\n".join(lines)


if __name__ == "__main__":
    import sr_amd
    print(baseline_table(sr_amd))
