"""Float64 statement of HaarPSI (piq 0.7.0 `haarpsi` / `HaarPSILoss` with their defaults), written in piq's own structure and
kept apart from the package's code: the tests compare sr_amd.haarpsi against it.

rgb2yiq as a matmul; subsampling by F.pad (bottom / right) + avg_pool2d; the Haar coefficients of each scale by one conv2d
with the stacked kernels (K, K^T); `similarity_map` with EPS; the logit squared.  The coefficient planes are kept in
orientation-major order (o0 s1, o0 s2, o0 s3, o1 s1, o1 s2, o1 s3), which is what piq's indexing
`scales - 1 + orientation * scales` (weights) and `(orientation * scales, 1 + orientation * scales)` (similarities) reads."""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -23            # piq's EPS inside the similarity, and finfo(fp32).eps in the score ratio
C, ALPHA, SCALES = 30.0, 4.2, 3

_YIQ = [[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]]


def rgb2yiq(x):
    m = torch.tensor(_YIQ, dtype=x.dtype, device=x.device).t()
    return torch.matmul(x.permute(0, 2, 3, 1), m).permute(0, 3, 1, 2)


def haar_filter(k, dtype):
    kernel = torch.ones((k, k), dtype=dtype) / k
    kernel[k // 2:, :] = -kernel[k // 2:, :]
    return kernel.unsqueeze(0)


def haar_wavelet_decompose(x, scales=SCALES):
    """(N, 1, H, W) -> (N, 2 * scales, H, W), orientation-major."""
    per_scale = []
    for s in range(1, scales + 1):
        k = 2 ** s
        kernels = torch.stack([haar_filter(k, x.dtype), haar_filter(k, x.dtype).transpose(-1, -2)]).to(x.device)
        upper, bottom = k // 2 - 1, k // 2
        per_scale.append(F.conv2d(F.pad(x, pad=[upper, bottom, upper, bottom], mode="constant"), kernels))
    return torch.cat([c[:, o:o + 1] for o in range(2) for c in per_scale], dim=1)


def similarity_map(map_x, map_y, constant):
    return (2.0 * map_x * map_y + constant) / (map_x ** 2 + map_y ** 2 + constant + EPS)


def haarpsi_index(x, y):
    """Per-batch HaarPSI index (mean over images) of test image x against reference y, N x C x H x W, data_range 1.  No
    clamp: the caller clamps x as the model does."""
    x, y = x.double() * 255.0, y.double() * 255.0
    if x.size(-1) < 2 ** (SCALES + 1) or x.size(-2) < 2 ** (SCALES + 1):
        raise ValueError("image too small")
    n_ch = x.size(1)
    if n_ch == 3:
        x_yiq, y_yiq = rgb2yiq(x), rgb2yiq(y)
    else:
        x_yiq, y_yiq = x, y
    p = max(x.shape[2] % 2, x.shape[3] % 2)
    x_yiq = F.avg_pool2d(F.pad(x_yiq, pad=[0, p, 0, p]), kernel_size=2, stride=2, padding=0)
    y_yiq = F.avg_pool2d(F.pad(y_yiq, pad=[0, p, 0, p]), kernel_size=2, stride=2, padding=0)
    cx = haar_wavelet_decompose(x_yiq[:, :1])
    cy = haar_wavelet_decompose(y_yiq[:, :1])
    orientations = 3 if n_ch == 3 else 2
    weights = torch.zeros_like(cx[:, :orientations])
    sims = torch.zeros_like(cx[:, :orientations])
    for o in range(2):
        weights[:, o] = torch.max(torch.abs(cx[:, SCALES - 1 + o * SCALES]), torch.abs(cy[:, SCALES - 1 + o * SCALES]))
        mx = torch.abs(cx[:, (o * SCALES, 1 + o * SCALES)])
        my = torch.abs(cy[:, (o * SCALES, 1 + o * SCALES)])
        sims[:, o] = similarity_map(mx, my, C).sum(dim=1) / 2
    if n_ch == 3:
        xi = F.avg_pool2d(F.pad(x_yiq[:, 1:], pad=[0, 1, 0, 1]), kernel_size=2, stride=1, padding=0)
        yi = F.avg_pool2d(F.pad(y_yiq[:, 1:], pad=[0, 1, 0, 1]), kernel_size=2, stride=1, padding=0)
        sims[:, 2] = similarity_map(torch.abs(xi), torch.abs(yi), C).sum(dim=1) / 2
        weights[:, 2] = weights[:, :2].mean(dim=1)
    r = ((torch.sigmoid(sims * ALPHA) * weights).sum(dim=[1, 2, 3]) + EPS) / (torch.sum(weights, dim=[1, 2, 3]) + EPS)
    score = (torch.log(r / (1 - r)) / ALPHA) ** 2
    return score.mean()


def haarpsi_loss(sr, hr):
    """HaarPSILoss as the reference's model calls it: 1 - index(clamp(sr, 0, 1), hr)."""
    return 1.0 - haarpsi_index(sr.clamp(0, 1), hr)
