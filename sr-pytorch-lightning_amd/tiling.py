"""Tiled and x8 self-ensemble inference for images of any size (INTEGRATION.md "Large images and self-ensemble").

Tiling, per spatial axis independently (LR length L, tile side T, pad P, T > 2P >= 0):
  * L <= T: one tile, start 0, length L;
  * else stride = T - 2P, n = ceil((L - T) / stride) + 1 tiles of length T at s_i = min(i * stride, L - T) (the last one is shifted
    inwards, not padded);
  * ownership boundaries b_0 = 0, b_n = L, b_i = (s_{i-1} + T + s_i) // 2: tile i owns LR positions [b_i, b_{i+1}), and the same
    interval times `scale` of the HR image.  Every output pixel is written exactly once, from its owner; nothing is blended.
An owned pixel that is not at the image border lies at least P LR pixels inside its tile, and at the image border the tile's edge is the
image's edge, so a purely convolutional model of receptive radius <= P gives the whole-image result (in exact arithmetic).  RCAN's
channel attention pools over the tile: its tiled result is well defined but not the whole-image one.

Self-ensemble: transform k in 0..7 -- bit 0 reverses W, bit 1 reverses H, bit 2 transposes H and W after the flips -- and
result = 0.125 * sum_k inverse_k(f(transform_k(x))), summed in fp32 in the order k = 0..7 (as out += 0.125 * v_k: the factor is a power
of two, so this is the same number).  The ensemble is the outer operation: each TRANSFORMED image is tiled by the rule above, i.e. the
grid is planned on transform_k(x)'s own sides (`plan(W, H, ...)` for the transposed ids) and a tile is a rectangle of transform_k(x).
Transformed tiles of the untransformed grid would not be the same thing: the inward-shifted last tile of an axis sits at the END of the
transformed axis, which for a reversed axis is the image's beginning.

On CUDA the tiles of a batch are cut and transformed by ONE launch (srk_tile_gather), the SR tiles are transformed back and written (or
accumulated) into the HR image by ONE launch per transform id of the batch (srk_tile_place), and the table of (origin, id, owned
rectangle) per tile is uploaded once per image.  Elsewhere the same values come from torch slicing, `flip` and `transpose`, in the
input's dtype (fp32 or float64), for any callable.
"""
import ctypes
from dataclasses import dataclass

import torch

# EDSR-baseline x4 reads 36 LR pixels to each side of an output pixel (head 1 + 16 ResBlocks x 2 + body conv 1 + the upsampler's convs at
# LR and 2x resolution 1 + 1/2 + the tail conv at HR 1/4, rounded up): with this pad its tiled image is the whole-image one
DEFAULT_TILE_PAD = 40
DEFAULT_TILE_BATCH = 64     # the fastest of {1, 4, 16, 64} measured ("Large images and self-ensemble", measurement 2)


def check_args(tile, pad, tile_batch):
    """The constructor's / `tiled_forward`'s refusals."""
    for name, v in (("tile", tile), ("tile_pad", pad), ("tile_batch", tile_batch)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an int, got {v!r}")
        if v < 0:
            raise ValueError(f"{name} must not be negative, got {v}")
    if tile_batch < 1:
        raise ValueError(f"tile_batch must be at least 1, got {tile_batch}")
    if tile and not tile > 2 * pad:
        raise ValueError(f"tile ({tile}) must exceed 2 * tile_pad ({2 * pad}): a tile has to own something")


def axis_plan(L, T, P):
    """-> (starts, tile length, boundaries): the module docstring's rule on one axis."""
    if L <= T:
        return [0], L, [0, L]
    stride = T - 2 * P
    n = -(-(L - T) // stride) + 1
    starts = [min(i * stride, L - T) for i in range(n)]
    bounds = [0] + [(starts[i - 1] + T + starts[i]) // 2 for i in range(1, n)] + [L]
    return starts, T, bounds


@dataclass(frozen=True)
class Tile:
    y0: int       # tile origin (LR)
    x0: int
    oy0: int      # owned LR rectangle [oy0, oy1) x [ox0, ox1); the HR one is this times `scale`
    oy1: int
    ox0: int
    ox1: int


@dataclass(frozen=True)
class Plan:
    H: int
    W: int
    scale: int
    th: int       # LR tile sides (min(H, tile), min(W, tile))
    tw: int
    tiles: tuple  # row-major over (tile row, tile column)

    def owned_hr(self, t):
        s = self.scale
        return t.oy0 * s, t.oy1 * s, t.ox0 * s, t.ox1 * s


def plan(H, W, scale, tile, pad):
    """Tile starts and owned rectangles of an H x W LR image.  `tile == 0`: one tile, the whole image."""
    if tile == 0:
        tile, pad = max(H, W), 0
    if not (H > 0 and W > 0 and scale > 0 and pad >= 0 and tile > 2 * pad):
        raise ValueError(f"plan(H={H}, W={W}, scale={scale}, tile={tile}, pad={pad})")
    ys, th, by = axis_plan(H, tile, pad)
    xs, tw, bx = axis_plan(W, tile, pad)
    tiles = tuple(Tile(y, x, by[i], by[i + 1], bx[j], bx[j + 1]) for i, y in enumerate(ys) for j, x in enumerate(xs))
    return Plan(H, W, scale, th, tw, tiles)


def transform(x, k):
    """transform_k on the last two axes."""
    if k & 1:
        x = x.flip(-1)
    if k & 2:
        x = x.flip(-2)
    if k & 4:
        x = x.transpose(-1, -2)
    return x


def inverse(y, k):
    """inverse_k: inverse(transform(x, k), k) is x."""
    if k & 4:
        y = y.transpose(-1, -2)
    if k & 2:
        y = y.flip(-2)
    if k & 1:
        y = y.flip(-1)
    return y


def _frame_rect_to_image(k, sH, sW, r0, r1, c0, c1):
    """Rows [r0, r1) x columns [c0, c1) of transform_k(image) -> (y, x, h, w) of that rectangle in the sH x sW image."""
    if k & 4:
        r0, r1, c0, c1 = c0, c1, r0, r1
    if k & 2:
        r0, r1 = sH - r1, sH - r0
    if k & 1:
        c0, c1 = sW - c1, sW - c0
    return r0, c0, r1 - r0, c1 - c0


def _plans(H, W, scale, tile, pad, self_ensemble):
    """[(k, plan of transform_k(x))] in the order of the sum."""
    return [(k, plan(W, H, scale, tile, pad) if k & 4 else plan(H, W, scale, tile, pad)) for k in (range(8) if self_ensemble else (0,))]


def _check_tiles(y, nb, C, sth, stw):
    if tuple(y.shape) != (nb, C, sth, stw):
        raise ValueError(f"tiled_forward: fn returned {tuple(y.shape)} for a batch of {nb} tiles, expected {(nb, C, sth, stw)}")


def device_table(plans, H, W):
    """The ctypes table of every entry of `plans` (in order) for an H x W LR image, and per plan its first entry's index."""
    from . import _lib as L
    descs, first = [], []
    for k, p in plans:
        first.append(len(descs))
        s = p.scale
        for t in p.tiles:
            oy, ox, oh, ow = _frame_rect_to_image(k, H * s, W * s, *p.owned_hr(t))
            descs.append(L.TileDesc(y0=t.y0, x0=t.x0, id=k, oy=oy, ox=ox, oh=oh, ow=ow, pad_=0))
    return (L.TileDesc * len(descs))(*descs), first


def gather(x, table, first, n, th, tw):
    """srk_tile_gather: entries [first, first + n) of the DEVICE table (a uint8 tensor of TileDesc) cut out of x [1, C, H, W] fp32."""
    from . import _lib as L, packing
    _, C, H, W = x.shape
    out = torch.empty(n, C, th, tw, dtype=torch.float32, device=x.device)
    a = L.TileArgs(src=x.data_ptr(), dst=out.data_ptr(), table=table.data_ptr() + first * ctypes.sizeof(L.TileDesc),
                   N=n, C=C, H=H, W=W, th=th, tw=tw, scale=1, max_oh=0, max_ow=0, accumulate=0, weight=0.0)
    L.call("srk_tile_gather", a, packing._stream())
    return out


def place(y, out, table, first, n, lr_hw, th, tw, scale, max_oh, max_ow, weight=None):
    """srk_tile_place: SR tiles y [n, C, scale*th, scale*tw] fp32 -> the owned rectangles of entries [first, first + n) of `out`
    [1, C, scale*H, scale*W]; `weight` None stores, a float accumulates out += weight * v."""
    from . import _lib as L, packing
    C = out.shape[1]
    H, W = lr_hw
    assert y.dtype == torch.float32 and y.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous()
    assert tuple(y.shape) == (n, C, scale * th, scale * tw) and tuple(out.shape) == (1, C, scale * H, scale * W)
    a = L.TileArgs(src=y.data_ptr(), dst=out.data_ptr(), table=table.data_ptr() + first * ctypes.sizeof(L.TileDesc),
                   N=n, C=C, H=H, W=W, th=th, tw=tw, scale=scale, max_oh=max_oh, max_ow=max_ow,
                   accumulate=int(weight is not None), weight=float(weight or 0.0))
    L.call("srk_tile_place", a, packing._stream())


def _forward_cuda(fn, x, plans, tile_batch, ens):
    from . import packing
    _, C, H, W = x.shape
    s = plans[0][1].scale
    host, first = device_table(plans, H, W)
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(x.device)      # once per image
    out = (torch.zeros if ens else torch.empty)(1, C, H * s, W * s, dtype=torch.float32, device=x.device)
    # a batch: consecutive entries of ONE tile shape (the transposed ids of a non-square grid have their own), at most tile_batch of them.
    # One gather per batch; one place per transform id inside it, in table order, so that every pixel's sum runs k = 0..7
    runs = [(k, f, len(p.tiles), p.th, p.tw) for (k, p), f in zip(plans, first)]
    i = 0
    while i < len(runs):
        j = i
        while j < len(runs) and runs[j][3:] == runs[i][3:]:
            j += 1
        th, tw = runs[i][3:]
        begin, end = runs[i][1], runs[j - 1][1] + runs[j - 1][2]
        for b0 in range(begin, end, tile_batch):
            nb = min(tile_batch, end - b0)
            y = fn(gather(x, table, b0, nb, th, tw))
            _check_tiles(y, nb, C, s * th, s * tw)
            y = packing._f32c(y)
            for k, f, n, _, _ in runs[i:j]:
                lo, hi = max(b0, f), min(b0 + nb, f + n)
                if lo < hi:
                    ent = host[lo:hi]
                    place(y[lo - b0:hi - b0], out, table, lo, hi - lo, (H, W), th, tw, s, max(e.oh for e in ent), max(e.ow for e in ent),
                          weight=0.125 if ens else None)
        i = j
    return out


def _forward_torch(fn, x, plans, tile_batch, ens):
    _, C, H, W = x.shape
    s = plans[0][1].scale
    out = None
    for k, p in plans:
        xk = transform(x, k)
        canvas = None
        for b0 in range(0, len(p.tiles), tile_batch):
            ts = p.tiles[b0:b0 + tile_batch]
            y = fn(torch.cat([xk[:, :, t.y0:t.y0 + p.th, t.x0:t.x0 + p.tw] for t in ts]).contiguous())
            _check_tiles(y, len(ts), C, s * p.th, s * p.tw)
            if canvas is None:
                canvas = torch.empty(1, C, p.H * s, p.W * s, dtype=y.dtype, device=y.device)
            for n, t in enumerate(ts):
                r0, r1, c0, c1 = p.owned_hr(t)
                canvas[0, :, r0:r1, c0:c1] = y[n, :, r0 - t.y0 * s:r1 - t.y0 * s, c0 - t.x0 * s:c1 - t.x0 * s]
        v = inverse(canvas, k)
        if not ens:
            return v.contiguous()
        out = torch.zeros_like(v, memory_format=torch.contiguous_format) if out is None else out
        out += 0.125 * v
    return out


def tiled_forward(fn, x, scale, tile=0, pad=DEFAULT_TILE_PAD, tile_batch=DEFAULT_TILE_BATCH, self_ensemble=False):
    """`fn` (N x C x h x w -> N x C x scale*h x scale*w) applied to x [N, C, H, W] tile by tile and / or as the mean over the 8
    transforms: the module docstring's definition.  `tile == 0`: no tiling (each transformed image is one tile).  Images of a batch are
    processed one after the other.  CUDA: x is read as fp32, the result is fp32; elsewhere the result has fn's dtype."""
    check_args(tile, pad, tile_batch)
    if x.dim() != 4:
        raise ValueError(f"tiled_forward expects N x C x H x W, got {tuple(x.shape)}")
    if tile == 0:
        pad = 0
    N, _, H, W = x.shape
    plans = _plans(H, W, scale, tile, pad, self_ensemble)
    if x.is_cuda:
        x = x.float().contiguous()
        run = _forward_cuda
    else:
        run = _forward_torch
    outs = [run(fn, x[n:n + 1], plans, tile_batch, self_ensemble) for n in range(N)]
    return outs[0] if N == 1 else torch.cat(outs)
