"""Float64 statement of the MS-SSIM loss (piq.MultiScaleSSIMLoss with piq.multi_scale_ssim's defaults), kept apart from the
package's code: the tests compare sr_amd.ms_ssim_loss against it, and its gradient is torch autograd's.

Deliberately not the product's form: the Gaussian is ONE dense 11 x 11 conv2d per moment (the product filters rows, then
columns, of images shifted by 1/2), every plane goes through the conv as its own batch entry, the pyramid is F.pad + F.avg_pool2d,
and the rule for a level mean <= 0 (value 0, gradient 0: where piq's relu(m) ** w gives a NaN gradient) is an explicit mask over the
planes."""
import torch
import torch.nn.functional as F

from ssim_loss_ref import gauss2d, images  # noqa: F401  (the input recipe of the loss tests; `images` is re-exported)

KERNEL_SIZE, K1, K2 = 11, 0.01, 0.03
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIZE = (KERNEL_SIZE - 1) * 2 ** (len(WEIGHTS) - 1) + 1          # 161


def level_means(x, y):
    """[5, N, C] float64: per level and plane the mean the product uses, cs_k for k < 4 and ss_4 for the last level."""
    if x.dim() != 4 or x.shape != y.shape or min(x.shape[-2:]) < MIN_SIZE:
        raise ValueError(f"Invalid size of the input images, expected at least {MIN_SIZE}x{MIN_SIZE}.")
    x, y = x.double(), y.double()
    k = gauss2d()
    c1, c2 = K1 ** 2, K2 ** 2
    out = []
    for level in range(len(WEIGHTS)):
        if level > 0:
            p = max(x.shape[-2] % 2, x.shape[-1] % 2)
            x = F.avg_pool2d(F.pad(x, [p, 0, p, 0], mode="replicate"), kernel_size=2, stride=2)
            y = F.avg_pool2d(F.pad(y, [p, 0, p, 0], mode="replicate"), kernel_size=2, stride=2)
        n, c, h, w = x.shape
        conv = lambda t: F.conv2d(t.reshape(n * c, 1, h, w), k)         # noqa: E731
        mu_x, mu_y = conv(x), conv(y)
        s_xx = conv(x * x) - mu_x ** 2
        s_yy = conv(y * y) - mu_y ** 2
        s_xy = conv(x * y) - mu_x * mu_y
        m = (2.0 * s_xy + c2) / (s_xx + s_yy + c2)
        if level == len(WEIGHTS) - 1:
            m = (2.0 * mu_x * mu_y + c1) / (mu_x ** 2 + mu_y ** 2 + c1) * m
        out.append(m.reshape(n, c, -1).mean(dim=2))
    return torch.stack(out)


def ms_ssim_index(x, y):
    """MS-SSIM (mean over images of the mean over channels of prod_k m_k^w_k).  A plane with any m_k <= 0 contributes the constant
    0: no gradient flows from it.  No clamp: the caller clamps x as the model does."""
    m = level_means(x, y)
    dead = (m <= 0).any(dim=0)                                          # [N, C]
    v = torch.zeros_like(m[0])
    live = ~dead
    if live.any():
        logs = sum(w * torch.log(m[k][live]) for k, w in enumerate(WEIGHTS))
        v = v.masked_scatter(live, torch.exp(logs))
    return v.mean(dim=1).mean()


def ms_ssim_loss(sr, hr):
    """MultiScaleSSIMLoss as the model calls its piq losses: 1 - index(clamp(sr, 0, 1), hr)."""
    return 1.0 - ms_ssim_index(sr.clamp(0, 1), hr)


def loss_and_grad(sr, hr):
    """(loss, d loss / d sr) of the float64 statement."""
    s = sr.detach().double().requires_grad_(True)
    loss = ms_ssim_loss(s, hr.double())
    loss.backward()
    return loss.detach(), s.grad


def anticorrelated(seed, shape=(1, 3, 161, 161)):
    """(sr, hr): plane (0, 0) has sr = 1 - hr on a textured hr (its contrast-structure means are negative), the other planes are
    the `images` recipe's."""
    sr, hr = images(shape, seed, spill=False)
    g = torch.Generator().manual_seed(seed + 1000)
    hr[0, 0] = torch.rand(shape[-2:], generator=g)
    sr[0, 0] = 1.0 - hr[0, 0]
    return sr, hr


# the shapes every comparison with this statement runs at: the minimum size (every level odd and padded, level 4 a single map
# position); all levels even; H even and W odd (p = 1 pads both axes, the last padded row is dropped); a dropped column;
# non-square with mixed parity down the levels (82x105, 41x53, 21x27, 11x14); the training patch (several tiles per level)
SHAPES = [(1, 1, 161, 161), (1, 1, 176, 176), (2, 3, 162, 161), (1, 2, 161, 176), (1, 1, 163, 209), (2, 3, 192, 192)]
# what the HIP path must keep against this statement on `images`: |d loss|, the gradient's relative L2 error, and its largest
# element-wise error over the largest gradient entry.  Set from what `ms_ssim_torch` in fp32 costs on these inputs
# (tests/test_ms_ssim_loss_cpu.py measures it and asserts a threefold margin); they are the SSIM loss's limits.
LIMIT_LOSS, LIMIT_L2, LIMIT_MAX = 1e-5, 1e-3, 3e-3


def errors(loss, grad, loss64, grad64):
    g = grad.detach().cpu().double()
    return (abs(float(loss) - float(loss64)), float((g - grad64).norm() / grad64.norm()),
            float((g - grad64).abs().max()) / float(grad64.abs().max()))
