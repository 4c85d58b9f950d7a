"""Float64 statement of the GMSD loss (piq.GMSDLoss: gradient magnitude similarity deviation, Xue, Zhang, Mou, Bovik 2014), kept
apart from the package's code: the tests compare sr_amd.gmsd against it, and its gradient is torch autograd's.

Deliberately not the product's form: the two Prewitt taps are ONE dense 2-channel conv2d (the product takes differences of shifted
planes), GMS is written as piq writes it, (2ab + c) / (a^2 + b^2 + c) (the product works with GMS - 1 = -(a - b)^2 / (...)), the
deviation is torch.var's, the two zero cases are torch.where guards, and nothing is tiled.

The definition (x = clamp(sr, 0, 1) the test image, y = hr the reference, N x C x H x W, C = 1 or 3):
  luma 0.299 R + 0.587 G + 0.114 B (C = 3);  p = max(H % 2, W % 2) rows / columns of zeros at the bottom / right, then the 2 x 2
  average with stride 2 and floor;  kx = [[-1, 0, 1]] x 3 / 3, ky = kx^T, cross-correlation with zero padding 1;  a, b = the gradient
  magnitudes of x, y;  GMS = (2ab + c) / (a^2 + b^2 + c), c = 170 / 255^2;  GMSD_n = the population standard deviation of GMS over
  the map of image n;  loss = mean over n of GMSD_n.
  Gradient: where gx = gy = 0 the square root's derivative is 0; an image whose variance of GMS is exactly 0 gets a zero gradient."""
import torch
import torch.nn.functional as F

from ssim_loss_ref import images as _images

C_GMS = 170.0 / 255.0 ** 2


def prewitt(dtype=torch.float64):
    """3 kx and 3 ky as one [2][1][3][3] weight.  The taps are kept whole and the 1/3 is applied to the result: every product is
    then exact, so a flat neighbourhood gives gx = gy = 0 exactly, as the definition's zero case needs (with taps of 1/3 a fused
    multiply-add leaves 1e-17 there, and the square root's derivative turns that into a gradient of full size)."""
    kx = torch.tensor([[-1.0, 0.0, 1.0]] * 3, dtype=dtype)
    return torch.stack((kx, kx.t())).unsqueeze(1)


def gradient_magnitude(t):
    """sqrt(gx^2 + gy^2) of the pooled luma of t (N x C x H x W), N x Hd x Wd, in t's dtype; the derivative at gx = gy = 0 is 0."""
    if t.shape[1] == 3:
        t = (t * torch.tensor([0.299, 0.587, 0.114], dtype=t.dtype).view(1, 3, 1, 1)).sum(dim=1, keepdim=True)
    elif t.shape[1] != 1:
        raise ValueError("1 or 3 channels")
    p = max(t.shape[-2] % 2, t.shape[-1] % 2)
    t = F.avg_pool2d(F.pad(t, [0, p, 0, p], mode="constant", value=0.0), kernel_size=2, stride=2)
    g = F.conv2d(t, prewitt(t.dtype), padding=1) / 3.0
    s = (g ** 2).sum(dim=1)
    flat = s == 0
    return torch.where(flat, torch.zeros_like(s), torch.sqrt(torch.where(flat, torch.ones_like(s), s)))


def gmsd_index(x, y, dtype=torch.float64):
    """GMSD (mean over images of the deviation of the GMS map) of test image x against reference y.  No clamp: the caller clamps x
    as the model does.  `dtype`: float64 is the statement; float32 measures what fp32 arithmetic alone costs it."""
    a, b = gradient_magnitude(x.to(dtype)), gradient_magnitude(y.to(dtype))
    gms = (2.0 * a * b + C_GMS) / (a ** 2 + b ** 2 + C_GMS)
    var = torch.var(gms.flatten(1), dim=1, unbiased=False)
    same = var == 0
    return torch.where(same, torch.zeros_like(var), torch.sqrt(torch.where(same, torch.ones_like(var), var))).mean()


def gmsd_loss(sr, hr, dtype=torch.float64):
    """GMSDLoss as the model calls its piq losses: index(clamp(sr, 0, 1), hr)."""
    return gmsd_index(sr.clamp(0, 1), hr, dtype)


def images(shape, seed, spill=True):
    """The input recipe of the loss tests (ssim_loss_ref.images); with more than one image the first SR image is its reference, so
    every multi-image case carries an image of zero variance."""
    sr, hr = _images(shape, seed, spill)
    if shape[0] > 1:
        sr[0] = hr[0]
    return sr, hr


def loss_and_grad(sr, hr, dtype=torch.float64):
    """(loss, d loss / d sr) of the statement, in float64 unless told otherwise."""
    s = sr.detach().to(dtype).requires_grad_(True)
    loss = gmsd_loss(s, hr.to(dtype), dtype)
    loss.backward()
    return loss.detach(), s.grad


# The shapes every comparison with this statement runs at.  The kernels tile the pooled map 16 x 32 (forward and backward: 32 x 64
# pixels of sr): one pooled position (loss 0); 2 x 2 positions; the zero pad at the bottom (5 x 4: both sizes pad, the pad column is
# dropped) and at the right (4 x 5); one tile exactly (32 x 64) and one position more each way (34 x 66); two tiles each way with
# odd H and odd W, C = 1, the zero-variance image first (37 x 71); N > 1 with C = 3; the training patch; a non-square image with
# both sizes odd (several tiles, the pad row and column in partial tiles).
SHAPES = [(1, 1, 2, 2), (1, 1, 4, 4), (1, 3, 5, 4), (1, 3, 4, 5), (1, 1, 32, 64), (1, 3, 34, 66), (2, 1, 37, 71), (3, 3, 48, 40),
          (16, 3, 192, 192), (1, 3, 203, 331)]
# What the HIP path must keep against this statement on `images`: |d loss|, the gradient's relative L2 error, and its largest
# element-wise error over the largest gradient entry.  Ten times what THIS statement run in fp32 costs against itself in float64 on
# these shapes (tests/test_gmsd_cpu.py::test_fp32_reference_statement_sets_the_limits measures the floors and holds them to a third
# of the limits): the floors are FLOOR_*; the margin is for the kernel's summation order and its square root and division.  All
# three are tighter than the SSIM loss's (1e-5, 1e-3, 3e-3).
FLOOR_LOSS, FLOOR_L2, FLOOR_MAX = 2.7e-8, 8.2e-6, 1.1e-5
LIMIT_LOSS, LIMIT_L2, LIMIT_MAX = 2.7e-7, 8.2e-5, 1.1e-4


def errors(loss, grad, loss64, grad64):
    """(|d loss|, relative L2, max error over the largest entry); a zero reference gradient (one pooled position) asks for zero."""
    g = grad.detach().cpu().double()
    if float(grad64.abs().max()) == 0.0:
        z = float(g.abs().max())
        return abs(float(loss) - float(loss64)), z, z
    return (abs(float(loss) - float(loss64)), float((g - grad64).norm() / grad64.norm()),
            float((g - grad64).abs().max()) / float(grad64.abs().max()))
