"""Float64 statement of the pixel losses (Charbonnier, Huber, smooth-L1, Barron's general robust loss with fixed alpha and c, the PSNR
loss), kept apart from the package's code: the tests compare sr_amd.pixel_loss against it, and its gradient is torch autograd's.

With d = sr - hr, mean reduction over every element, nothing clamped:
  charbonnier   sqrt(d^2 + eps^2)
  huber         d^2 / 2 if |d| <= delta, else delta (|d| - delta / 2)
  smooth_l1     d^2 / (2 beta) if |d| < beta, else |d| - beta / 2; beta = 0: |d|
  robust        Barron, CVPR 2019, eq. 13: z = (d / c)^2, b = |alpha - 2|; alpha = 2: z / 2; alpha = 0: log1p(z / 2); alpha = -inf:
                -expm1(-z / 2); otherwise (b / alpha) expm1((alpha / 2) log1p(z / b)) -- the form that keeps its digits for small |d|
  psnr          (10 / ln 10) mean over images of ln(mse_n + eps), mse_n the mean of d^2 over image n"""
import math
import os
import re

import torch

_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srk.h")).read()
#: elements one block of the elementwise kernels covers per pass, and the most blocks a launch has (include/srk.h)
BLOCK_ELEMS = int(re.search(r"#define SRK_PIXEL_LOSS_BLOCK_ELEMS (\d+)", _HEADER).group(1))
BLOCKS_MAX = int(re.search(r"#define SRK_PIXEL_LOSS_BLOCKS_MAX (\d+)", _HEADER).group(1))


def charbonnier(sr, hr, eps=1e-3):
    d = sr - hr
    return torch.sqrt(d ** 2 + eps ** 2).mean()


def huber(sr, hr, delta=1.0):
    d = sr - hr
    return torch.where(d.abs() <= delta, d ** 2 / 2, delta * (d.abs() - delta / 2)).mean()


def smooth_l1(sr, hr, beta=1.0):
    d = sr - hr
    if beta == 0:
        return d.abs().mean()
    return torch.where(d.abs() < beta, d ** 2 / (2 * beta), d.abs() - beta / 2).mean()


def robust(sr, hr, alpha, c):
    z = ((sr - hr) / c) ** 2
    if alpha == 2:
        rho = z / 2
    elif alpha == 0:
        rho = torch.log1p(z / 2)
    elif alpha == -math.inf:
        rho = -torch.expm1(-z / 2)
    else:
        b = abs(alpha - 2)
        rho = (b / alpha) * torch.expm1((alpha / 2) * torch.log1p(z / b))
    return rho.mean()


def psnr(sr, hr, eps=1e-8):
    d = (sr - hr).reshape(sr.shape[0], -1)
    return (10.0 / math.log(10.0)) * torch.log((d ** 2).mean(dim=1) + eps).mean()


STATEMENTS = {"charbonnier": charbonnier, "huber": huber, "smooth_l1": smooth_l1, "robust": robust, "psnr": psnr}


def loss_and_grad(kind, sr, hr, params, dtype=torch.float64):
    """(loss, d loss / d sr) of the statement of `kind`, in float64 unless told otherwise (float32 measures what fp32 arithmetic
    alone costs it)."""
    s = sr.detach().to(dtype).requires_grad_(True)
    loss = STATEMENTS[kind](s, hr.to(dtype), **params)
    loss.backward()
    return loss.detach(), s.grad


def images(shape, seed):
    """A seeded fp32 pair: hr in [0, 1), sr = hr + e with e a mixture: exactly 0 on about an eighth of the pixels, about 1e-4 on a
    quarter, about 0.05 on most, outliers of +-1.5 on about 1 % (they leave [0, 1]: nothing clamps), and on about 2 % the pair
    (0.75, 0.25) or (0.25, 0.75): |d| = 0.5 exactly, the threshold of the Huber and smooth-L1 cases."""
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(shape, generator=g)
    u = torch.rand(shape, generator=g)
    r = torch.randn(shape, generator=g)
    sign = torch.where(r >= 0, torch.ones_like(r), -torch.ones_like(r))
    e = 0.05 * r
    e = torch.where(u < 3 / 8, 1e-4 * r, e)
    e = torch.where(u < 1 / 8, torch.zeros_like(r), e)
    e = torch.where(u >= 0.99, 1.5 * sign, e)
    sr = hr + e
    edge = (u >= 0.97) & (u < 0.99)
    hr = torch.where(edge, 0.5 - 0.25 * sign, hr)
    sr = torch.where(edge, 0.5 + 0.25 * sign, sr)
    return sr, hr


def psnr_images(shape, seed):
    """`images`; with more than one image the first SR image is its target (mse = 0: ln(eps) and a zero gradient)."""
    sr, hr = images(shape, seed)
    if shape[0] > 1:
        sr[0] = hr[0]
    return sr, hr


# The elementwise cases every comparison runs: (id, loss, parameters).  The Huber and smooth-L1 thresholds are the 0.5 that `images`
# places |d| on; robust takes the three exact alphas, alpha = 1 (sqrt(z + 1) - 1), a negative one and a non-special 0.5, each with a
# scale c below and above the typical |d|.
ROBUST_ALPHAS = (2.0, 1.0, 0.0, -2.0, -math.inf, 0.5)
ROBUST_CS = (0.01, 0.1)
CASES = ([("charbonnier", "charbonnier", {"eps": 1e-3}), ("huber", "huber", {"delta": 0.5}), ("smooth_l1", "smooth_l1", {"beta": 0.5})]
         + [(f"robust-a{a:g}-c{c:g}", "robust", {"alpha": a, "c": c}) for a in ROBUST_ALPHAS for c in ROBUST_CS])

# Elementwise shapes, each the smallest that reaches a distinct path of the kernels (float4 grid-stride loop, a scalar tail of n % 4 in
# block 0, one double per block): the tail alone (1 and 3 elements); 105 = 26 float4s and a tail of 1; 1,536 = two blocks, no tail; one
# block's span (BLOCK_ELEMS) less one, exactly, plus one; and one float4 and a tail of 3 beyond what the largest grid covers in one pass
# (BLOCKS_MAX blocks: the grid-stride loop's second trip), 8.4 MB per tensor.
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 3), (1, 3, 5, 7), (2, 3, 16, 16), (1, 1, 1, BLOCK_ELEMS - 1), (1, 1, 1, BLOCK_ELEMS),
          (1, 1, 1, BLOCK_ELEMS + 1), (1, 1, 1, BLOCK_ELEMS * BLOCKS_MAX + 4 + 3)]
# PSNR shapes (one or more blocks per image, a scalar head up to the next 16-byte boundary, float4s, a scalar tail): one element; 35
# elements per image, so images 1 and 2 start inside a float4; aligned images; more images than a grid dimension; an image longer
# than one block's span (33 * 33 = 1,089, odd: two blocks per image, heads of 3 and 2) among three; two images of 257 * 259 = 66,563
# elements: 66 blocks per image, from 64 on the finalize launch sums an image's partials with a wave instead of a thread.
PSNR_SHAPES = [(1, 1, 1, 1), (3, 1, 5, 7), (2, 3, 16, 16), (65538, 1, 2, 2), (3, 1, 33, 33), (2, 1, 257, 259)]
# The most images the PSNR kernels take: one block each, 2^24 - 1 blocks of 256 threads, the largest grid below 2^32 threads.
PSNR_MOST_IMAGES = (1 << 24) - 1
# Alphas at the edges of what fp32 holds (c = 0.1), by the kernel they must reach through `robust_loss` on the GPU: 2 - 1e-9 is 2 in
# fp32, 1e-300 is 0, -1e39 is -inf, 2^-126 is the smallest normal alpha (the general kind, b / alpha = 1.7e38); 1e-40 (subnormal in
# fp32) is not launched and computes in float64 torch.  The fp32 statement cannot hold most of these, so they take no
# part in the floors; the robust limits, calibrated on the representable alphas, hold for them.
EDGE_ALPHAS = [(2.0 - 1e-9, "ROBUST_A2"), (1e-300, "ROBUST_A0"), (-1e39, "ROBUST_NEG_INF"), (2.0 ** -126, "ROBUST_GENERAL"),
               (1e-40, None)]

# What the HIP path and the fp32 torch path must keep against this statement on `images`: the loss's relative error, the gradient's
# relative L2 error, and its largest element-wise error over the largest gradient entry.  Per loss, ten times what THIS statement run in
# fp32 torch on the CPU costs against itself in float64 on these same inputs, the worst over the loss's cases and shapes
# (tests/test_pixel_loss_cpu.py::test_fp32_reference_statement_sets_the_limits measures the floors and holds them to a third of the
# limits).  The factor ten is for the kernel's summation order, sqrtf, division, expm1f and log1pf.
#          loss      relative L2   max / largest
FLOORS = {
    "charbonnier": (6.5e-8, 5.9e-8, 1.8e-7),      # measured 6.45e-08 5.89e-08 1.76e-07
    "huber": (1.1e-7, 4.5e-8, 3.9e-8),            # measured 1.10e-07 4.43e-08 3.82e-08
    "smooth_l1": (1.1e-7, 4.5e-8, 3.9e-8),        # measured 1.10e-07 4.43e-08 3.82e-08
    "robust": (1.7e-7, 5.2e-7, 5.7e-7),           # measured 1.61e-07 5.11e-07 5.67e-07 (the worst of the 12 (alpha, c) cases)
    "psnr": (8.4e-8, 2.1e-7, 2.3e-7),             # measured 8.32e-08 2.09e-07 2.26e-07 (over PSNR_SHAPES)
}
LIMITS = {k: tuple(10.0 * f for f in v) for k, v in FLOORS.items()}
LIMIT_LOSS = {k: v[0] for k, v in LIMITS.items()}
LIMIT_L2 = {k: v[1] for k, v in LIMITS.items()}
LIMIT_MAX = {k: v[2] for k, v in LIMITS.items()}


def errors(loss, grad, loss64, grad64):
    """(relative error of the loss, relative L2 of the gradient, max error over the largest entry); a zero reference loss or gradient
    asks for zero."""
    g = grad.detach().cpu().double()
    l, l64 = float(loss), float(loss64)
    dl = abs(l - l64) / abs(l64) if l64 != 0.0 else abs(l)
    if float(grad64.abs().max()) == 0.0:
        z = float(g.abs().max())
        return dl, z, z
    return dl, float((g - grad64).norm() / grad64.norm()), float((g - grad64).abs().max()) / float(grad64.abs().max())
