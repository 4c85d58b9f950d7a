"""float64 statement of tiled and x8 self-ensemble inference -- TEST INFRASTRUCTURE, imports nothing from the product.

Tiling, per spatial axis independently (LR length L, tile side T, pad P, T > 2P >= 0):
  L <= T: one tile, start 0, length L.  Otherwise stride = T - 2P, n = ceil((L - T) / stride) + 1, starts s_i = min(i * stride, L - T),
  every tile of length T; boundaries b_0 = 0, b_n = L, b_i = (s_{i-1} + T + s_i) // 2; tile i owns [b_i, b_{i+1}), times `scale` in HR.
  Every output pixel is written once, from its owner.
Self-ensemble: transform k in 0..7, bit 0 reverses W, bit 1 reverses H, bit 2 transposes H and W after the flips;
  result = 0.125 * sum_k inverse_k(F(transform_k(x))) in the order k = 0..7, F = the tiled f: the transformed image is tiled.

Written per pixel row / column rather than per rectangle list, so that it shares no structure with the product's planner: `owner(L, T, P)`
names for every LR position the start of the tile that owns it.
"""
import math

import torch


def axis(L, T, P):
    """-> (starts, tile length, owner): owner[p] is the index of the tile that owns LR position p."""
    assert T > 2 * P >= 0 and L > 0
    if L <= T:
        return [0], L, [0] * L
    stride = T - 2 * P
    n = math.ceil((L - T) / stride) + 1
    starts = [min(i * stride, L - T) for i in range(n)]
    b = [0] + [(starts[i - 1] + T + starts[i]) // 2 for i in range(1, n)] + [L]
    owner = []
    for i in range(n):
        owner += [i] * (b[i + 1] - b[i])
    assert len(owner) == L
    return starts, T, owner


def transform(x, k):
    if k & 1:
        x = torch.flip(x, dims=[3])
    if k & 2:
        x = torch.flip(x, dims=[2])
    if k & 4:
        x = x.permute(0, 1, 3, 2)
    return x


def inverse(y, k):
    if k & 4:
        y = y.permute(0, 1, 3, 2)
    if k & 2:
        y = torch.flip(y, dims=[2])
    if k & 1:
        y = torch.flip(y, dims=[3])
    return y


def tiled(f, x, scale, tile, pad):
    """f on every tile of x [1, C, H, W] (one at a time), the owned pixels of each copied into the result.  tile == 0: f(x)."""
    x = x.double()
    if tile == 0:
        return f(x).double()
    _, C, H, W = x.shape
    ys, th, oy = axis(H, tile, pad)
    xs, tw, ox = axis(W, tile, pad)
    oy = torch.tensor(oy).repeat_interleave(scale)          # owner of every HR row / column
    ox = torch.tensor(ox).repeat_interleave(scale)
    out = torch.full((1, C, H * scale, W * scale), float("nan"), dtype=torch.float64)
    for i, y0 in enumerate(ys):
        rows = torch.nonzero(oy == i).flatten()
        for j, x0 in enumerate(xs):
            cols = torch.nonzero(ox == j).flatten()
            t = f(x[:, :, y0:y0 + th, x0:x0 + tw].contiguous()).double()
            assert tuple(t.shape) == (1, C, th * scale, tw * scale)
            out[:, :, rows[:, None], cols[None, :]] = t[:, :, (rows - y0 * scale)[:, None], (cols - x0 * scale)[None, :]]
    assert not bool(torch.isnan(out).any())
    return out


def forward(f, x, scale, tile=0, pad=0, self_ensemble=False):
    """The definition: x [1, C, H, W] -> [1, C, scale*H, scale*W] float64."""
    if not self_ensemble:
        return tiled(f, x, scale, tile, pad)
    acc = None
    for k in range(8):
        v = inverse(tiled(f, transform(x.double(), k), scale, tile, pad), k)
        acc = v if acc is None else acc + v
    return 0.125 * acc
