"""Float64 statement of MS-SSIM with piq.multi_scale_ssim's defaults -- TEST INFRASTRUCTURE, never imported by the product.

Restated from piq's published algorithm (piq itself is not a dependency; parity with it is unpinned, as for PSNR and SSIM):
five levels with scale weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); level 0 is the input and level k > 0 is level k-1
replicate-padded by p = max(H % 2, W % 2) pixels on the top and left only (F.pad(x, [p, 0, p, 0])), then F.avg_pool2d(2);
no initial average-pool.  Per level and (image, channel): the 11x11 Gaussian (sigma 1.5) SSIM and contrast-structure maps
over the valid region, averaged; v = prod_{k<4} relu(cs_k)^w_k * relu(ss_4)^w_4, mean over channels, then over images.
tests/test_ms_ssim_cpu.py checks the model's CPU path against it, tests/test_gpu_ms_ssim.py the HIP kernels."""
import torch
import torch.nn.functional as F

from oracle.metrics import _gauss_kernel

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIZE = (11 - 1) * 2 ** (len(WEIGHTS) - 1) + 1


def pyramid_shapes(h, w):
    """(H, W) of the five levels."""
    shapes = [(h, w)]
    for _ in range(len(WEIGHTS) - 1):
        p = max(h % 2, w % 2)
        h, w = (h + p) // 2, (w + p) // 2
        shapes.append((h, w))
    return shapes


def ms_ssim(x, y, *, sigma=1.5, k1=0.01, k2=0.03):
    """-> dict(value: 0-d float64, shapes: the levels' (H, W), cs / ss: [5, N, C] float64 per-level means)."""
    if x.shape != y.shape or min(x.shape[-2:]) < MIN_SIZE:
        raise ValueError(f"Invalid size of the input images, expected at least {MIN_SIZE}x{MIN_SIZE}.")
    x, y = x.double().cpu(), y.double().cpu()
    c = x.shape[1]
    k = _gauss_kernel(11, sigma).view(1, 1, 11, 11).repeat(c, 1, 1, 1)
    c1, c2 = k1 ** 2, k2 ** 2
    shapes, css, sss = [], [], []
    for level in range(len(WEIGHTS)):
        if level > 0:
            p = max(x.shape[-2] % 2, x.shape[-1] % 2)
            x = F.avg_pool2d(F.pad(x, [p, 0, p, 0], mode="replicate"), kernel_size=2, stride=2, padding=0)
            y = F.avg_pool2d(F.pad(y, [p, 0, p, 0], mode="replicate"), kernel_size=2, stride=2, padding=0)
        shapes.append(tuple(x.shape[-2:]))
        mx, my = F.conv2d(x, k, groups=c), F.conv2d(y, k, groups=c)
        sxx = F.conv2d(x * x, k, groups=c) - mx ** 2
        syy = F.conv2d(y * y, k, groups=c) - my ** 2
        sxy = F.conv2d(x * y, k, groups=c) - mx * my
        cs = (2 * sxy + c2) / (sxx + syy + c2)
        ss = (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1) * cs
        css.append(cs.mean(dim=(-1, -2)))
        sss.append(ss.mean(dim=(-1, -2)))
    cs, ss = torch.stack(css), torch.stack(sss)
    w = torch.tensor(WEIGHTS, dtype=torch.float64).view(-1, 1, 1)
    vals = torch.relu(torch.cat([cs[:-1], ss[-1:]], dim=0))
    v = torch.prod(vals ** w, dim=0)
    return {"value": v.mean(dim=1).mean(), "shapes": shapes, "cs": cs, "ss": ss}
