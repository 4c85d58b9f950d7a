"""Float64 statement of the frequency losses (`fft`: BasicSR's FFTLoss; `ffl`: the focal frequency loss of Jiang et al., ICCV 2021,
with patch_factor=1, ave_spectrum=False, log_matrix=False, batch_matrix=False), kept apart from the package's code: the tests compare
sr_amd.freq_loss against it, and its gradient is torch autograd's.

Deliberately not the product's form: the full spectrum (no Hermitian half), one complex-free pair of dense cos / sin matrices per
axis applied with einsum, nothing tiled.

The definition, with d = sr - hr (nothing clamped), per plane (n, c) of H x W:
  D[k, l] = sum_{h, w} d[h, w] e^{-2 pi i (k h / H + l w / W)};  at the self-conjugate bins (2k = 0 mod H and 2l = 0 mod W) Im D is 0
  by definition (d is real): set to 0, never a rounding residue; its sign is 0 in the gradient.
  fft:  L = (sum |Re D| + sum |Im D|) / (2 N C H W).
  ffl:  Do = D / sqrt(H W), q = |Do|^2, w = (q / q_max)^(alpha / 2), q_max the plane's maximum, w a constant of the gradient;
        L = sum w q / (N C H W); a plane with q_max = 0 has w = 0."""
import math

import torch


def _cos_sin(n, dtype):
    """cos, sin(2 pi ((j k) mod n) / n) as n x n matrices: the product reduced with integers, the angle in float64."""
    j = torch.arange(n, dtype=torch.int64)
    ang = 2.0 * math.pi * ((j[:, None] * j[None, :]) % n).double() / n
    return torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)


def structural(H, W):
    """H x W mask of the self-conjugate bins."""
    k, l = torch.arange(H), torch.arange(W)
    return ((2 * k) % H == 0)[:, None] & ((2 * l) % W == 0)[None, :]


def spectrum(d, dtype=torch.float64):
    """(Re D, Im D) of the planes of d (N x C x H x W), Im D zero at the self-conjugate bins."""
    d = d.to(dtype)
    H, W = d.shape[-2:]
    ch, sh = _cos_sin(H, dtype)
    cw, sw = _cos_sin(W, dtype)
    # e^{-i(a + b)} = (cos a cos b - sin a sin b) - i (sin a cos b + cos a sin b)
    re = torch.einsum("kh,nchw,wl->nckl", ch, d, cw) - torch.einsum("kh,nchw,wl->nckl", sh, d, sw)
    im = -(torch.einsum("kh,nchw,wl->nckl", sh, d, cw) + torch.einsum("kh,nchw,wl->nckl", ch, d, sw))
    return re, torch.where(structural(H, W), torch.zeros((), dtype=dtype), im)


def fft_loss(sr, hr, dtype=torch.float64):
    re, im = spectrum(sr.to(dtype) - hr.to(dtype), dtype)
    return (re.abs().sum() + im.abs().sum()) / (2 * re.numel())


def ffl_loss(sr, hr, alpha=1.0, dtype=torch.float64):
    re, im = spectrum(sr.to(dtype) - hr.to(dtype), dtype)
    q = (re ** 2 + im ** 2) / (re.shape[-2] * re.shape[-1])
    qmax = q.detach().amax(dim=(-2, -1), keepdim=True)
    dead = qmax == 0
    w = torch.where(dead, torch.zeros_like(q), (q.detach() / torch.where(dead, torch.ones_like(qmax), qmax)) ** (alpha / 2.0))
    return (w * q).sum() / q.numel()


def loss_and_grad(kind, sr, hr, alpha=1.0, dtype=torch.float64):
    """(loss, d loss / d sr) of the statement, in float64 unless told otherwise (float32 measures what fp32 arithmetic alone costs
    it)."""
    s = sr.detach().to(dtype).requires_grad_(True)
    loss = fft_loss(s, hr, dtype) if kind == "fft" else ffl_loss(s, hr, alpha, dtype)
    loss.backward()
    return loss.detach(), s.grad


# The shapes every comparison with this statement runs at: the transform is the identity (1 x 1); all four bins self-conjugate
# (2 x 2); both sizes odd, so no Nyquist bin (5 x 7); both even, four self-conjugate bins (8 x 6); exactly one 32 x 32 MFMA tile;
# one more and one fewer than a tile (33 x 31); ragged both ways with N > 1 (37 x 71); 48 x 40 with N, C > 1; the training patch at a
# small N; a non-square plane with several column blocks (100 x 260).
SHAPES = [(1, 1, 1, 1), (1, 1, 2, 2), (1, 3, 5, 7), (1, 1, 8, 6), (1, 3, 32, 32), (1, 3, 33, 31), (2, 1, 37, 71), (3, 3, 48, 40),
          (2, 3, 192, 192), (1, 3, 100, 260)]
TAU = 1e-3               # `images` pushes every non-structural component of D out to at least TAU rms(D)
MARGIN_MIN = 5e-4        # what every test input must keep after the rounding to fp32 (tests/test_freq_loss_cpu.py asserts it)


def _rms(re, im):
    return torch.sqrt((re ** 2 + im ** 2).mean(dim=(-2, -1), keepdim=True))


def margin(sr, hr):
    """The smallest |Re D| or |Im D| over the non-structural components of every plane with a non-zero spectrum, over that plane's
    rms of |D|, measured in float64 on the inputs as they are (inf when there is no such component)."""
    re, im = spectrum(sr.double() - hr.double())
    rms = _rms(re, im)
    live = (rms > 0).expand_as(re)
    free = ~structural(*re.shape[-2:]).expand_as(re)
    rel_re, rel_im = re.abs() / torch.where(rms > 0, rms, torch.ones_like(rms)), im.abs() / torch.where(rms > 0, rms, torch.ones_like(rms))
    parts = [rel_re[live], rel_im[live & free]]
    return min((float(p.min()) for p in parts if p.numel()), default=math.inf)


def images(shape, seed):
    """(sr, hr) in fp32 whose difference has no spectral component near zero, which is what makes the `fft` gradient testable:
    sign(D) flips wherever fp32 rounding exceeds a component's magnitude, and ONE flipped Hermitian pair moves the gradient by about
    4 / sqrt(H W) of its rms.  sr, hr uniform in [0, 1]; D = fft2(sr - hr) in float64; every non-structural real or imaginary
    component below TAU rms(D) is pushed out to +-TAU rms(D), keeping its sign (Re D is even and Im D odd under (k, l) ->
    (-k, -l), so the pushed spectrum is still that of a real image); inverted; sr = float32(hr + d').  `margin` re-measures on the
    rounded inputs."""
    g = torch.Generator().manual_seed(seed)
    sr, hr = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    D = torch.fft.fft2(sr.double() - hr.double())
    floor = TAU * _rms(D.real, D.imag)
    free = ~structural(*shape[-2:])

    def push(x, where):
        small = where & (x.abs() < floor) & (x != 0)
        return torch.where(small, torch.sign(x) * floor, x)

    D = torch.complex(push(D.real, torch.ones_like(free)), push(D.imag, free))
    d = torch.fft.ifft2(D).real
    return (hr.double() + d).float(), hr


def ffl_images(shape, seed):
    """`images`; with more than one image the first SR image is its target: the plane with q_max = 0."""
    sr, hr = images(shape, seed)
    if shape[0] > 1:
        sr[0] = hr[0]
    return sr, hr


def case(kind, shape):
    """The (sr, hr) every test of loss `kind` uses at `shape`."""
    return (images if kind == "fft" else ffl_images)(shape, 11 + sum(shape))


# What the HIP path (and the fp32 torch statements) must keep against this statement on `case`: |d loss| / |loss|, the gradient's
# relative L2 error, and its largest element-wise error over the largest gradient entry.  Ten times the floor: what THIS statement
# run in fp32 costs against itself in float64 over SHAPES (tests/test_freq_loss_cpu.py::test_fp32_statement_sets_the_limits measures
# the floors and holds them to a third of the limits); the margin is for the kernel's summation and tile order.
FLOOR = {"fft": (1.4e-7, 3.0e-7, 4.5e-7), "ffl": (1.2e-7, 5.7e-7, 8.4e-7)}
LIMIT = {kind: tuple(10.0 * f for f in floors) for kind, floors in FLOOR.items()}


def errors(loss, grad, loss64, grad64):
    """(|d loss| / |loss|, relative L2, max error over the largest entry); a zero reference asks for zero."""
    g = grad.detach().cpu().double()
    dl = abs(float(loss) - float(loss64))
    dl = dl / abs(float(loss64)) if float(loss64) != 0.0 else dl
    if float(grad64.abs().max()) == 0.0:
        z = float(g.abs().max())
        return dl, z, z
    return dl, float((g - grad64).norm() / grad64.norm()), float((g - grad64).abs().max()) / float(grad64.abs().max())
