"""Float64 statement of the SSIM loss (piq.SSIMLoss with piq.ssim's defaults), kept apart from the package's code: the tests
compare sr_amd.ssim_loss against it, and its gradient is torch autograd's.

Deliberately not the product's form: the Gaussian is ONE dense 11 x 11 conv2d per moment (the product filters rows, then
columns), every plane goes through the conv as its own batch entry, and the SSIM map is written as luminance x contrast-structure
like piq does."""
import torch
import torch.nn.functional as F

KERNEL_SIZE, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


def gauss2d():
    co = torch.arange(KERNEL_SIZE, dtype=torch.float64) - (KERNEL_SIZE - 1) / 2.0
    g = torch.exp(-(co ** 2) / (2.0 * SIGMA ** 2))
    k = torch.outer(g, g)
    return (k / k.sum()).view(1, 1, KERNEL_SIZE, KERNEL_SIZE)


def ssim_index(x, y):
    """SSIM (mean over images of the mean over channels of the mean valid map) of test image x against reference y,
    N x C x H x W, data range 1.  No clamp: the caller clamps x as the model does."""
    x, y = x.double(), y.double()
    f = max(1, round(min(x.shape[-2:]) / 256))
    if f > 1:
        x, y = F.avg_pool2d(x, kernel_size=f), F.avg_pool2d(y, kernel_size=f)
    if x.shape[-2] < KERNEL_SIZE or x.shape[-1] < KERNEL_SIZE:
        raise ValueError("image too small")
    n, c, h, w = x.shape
    k = gauss2d()
    conv = lambda t: F.conv2d(t.reshape(n * c, 1, h, w), k)         # noqa: E731
    c1, c2 = K1 ** 2, K2 ** 2
    mu_x, mu_y = conv(x), conv(y)
    s_xx = conv(x * x) - mu_x ** 2
    s_yy = conv(y * y) - mu_y ** 2
    s_xy = conv(x * y) - mu_x * mu_y
    cs = (2.0 * s_xy + c2) / (s_xx + s_yy + c2)
    lum = (2.0 * mu_x * mu_y + c1) / (mu_x ** 2 + mu_y ** 2 + c1)
    return (lum * cs).reshape(n, c, -1).mean(dim=2).mean(dim=1).mean()


def ssim_loss(sr, hr):
    """SSIMLoss as the model calls its piq losses: 1 - index(clamp(sr, 0, 1), hr)."""
    return 1.0 - ssim_index(sr.clamp(0, 1), hr)


def images(shape, seed, spill=True):
    """The input recipe of the loss tests (tests/test_gpu_haarpsi.py's): HR-like smooth images with fine texture and a saturated
    corner; SR = HR + noise, with one region pushed above 1 and one below 0 when `spill`."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    hr = F.interpolate(torch.rand(n, c, max(2, h // 8), max(2, w // 8), generator=g), size=(h, w), mode="bilinear", align_corners=False)
    hr = (hr + 0.15 * torch.rand(n, c, h, w, generator=g)).clamp(0, 1)
    hr[:, :, : h // 4, : w // 4] = 1.0
    sr = hr + 0.05 * torch.randn(n, c, h, w, generator=g)
    if spill:
        sr[:, :, h // 2:, : w // 3] += 0.3                 # a region pushed above 1
        sr[:, :, : h // 3, w // 2:] -= 0.3                 # and one below 0
    return sr, hr


def loss_and_grad(sr, hr):
    """(loss, d loss / d sr) of the float64 statement."""
    s = sr.detach().double().requires_grad_(True)
    loss = ssim_loss(s, hr.double())
    loss.backward()
    return loss.detach(), s.grad


# the shapes every comparison with this statement runs at: a single valid position; one 16 x 16 map tile exactly and one more;
# odd sizes with several tiles either way; the training patch; f = 2 with a remainder column; f = 3 with remainders both ways
SHAPES = [(1, 3, 11, 11), (1, 1, 26, 26), (1, 1, 27, 27), (2, 3, 27, 38), (2, 1, 38, 27), (3, 2, 33, 33), (16, 3, 192, 192),
          (1, 1, 384, 391), (1, 1, 641, 644)]
# what the HIP path must keep against this statement on `images`: |d loss|, the gradient's relative L2 error, and its largest
# element-wise error over the largest gradient entry
LIMIT_LOSS, LIMIT_L2, LIMIT_MAX = 1e-5, 1e-3, 3e-3


def errors(loss, grad, loss64, grad64):
    g = grad.detach().cpu().double()
    return (abs(float(loss) - float(loss64)), float((g - grad64).norm() / grad64.norm()),
            float((g - grad64).abs().max()) / float(grad64.abs().max()))
