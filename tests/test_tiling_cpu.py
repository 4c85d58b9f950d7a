"""CPU tests of tiled and x8 self-ensemble inference (sr_amd.tiling, SRModel(tile=..., self_ensemble=...), predict.py --tile ...):
the planner's properties, the product's torch path against the independent float64 statement (tests/tiling_ref.py), the exactness claim
(pad >= receptive radius: tiled == whole; pad 0: a visible seam), the ensemble's identities, argument validation and predict.py end to end."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiling_ref as TR  # noqa: E402
from oracle import functional as OF  # noqa: E402

EPS64 = 2.0 ** -52


@pytest.fixture(scope="module")
def T():
    import sr_amd
    from sr_amd import tiling
    return tiling


# L < T, L == T, L == T + 1, L no multiple of the stride, L - T a multiple of the stride, P == 0, stride 1
GRID = [(L, T_, P) for T_, P in ((24, 8), (24, 0), (8, 2), (7, 3), (5, 0), (48, 8)) for L in (1, T_ - 1, T_, T_ + 1, T_ + (T_ - 2 * P), 45, 59, 100)]


@pytest.mark.parametrize("L,T_,P", GRID)
def test_axis_plan_properties(T, L, T_, P):
    starts, length, b = T.axis_plan(L, T_, P)
    n = len(starts)
    if L <= T_:
        assert (starts, length, b) == ([0], L, [0, L])
        return
    stride = T_ - 2 * P
    assert n == -(-(L - T_) // stride) + 1 and length == T_
    assert starts == [min(i * stride, L - T_) for i in range(n)] and starts[-1] == L - T_
    # the owned intervals partition [0, L)
    assert b[0] == 0 and b[-1] == L and len(b) == n + 1 and all(b[i] < b[i + 1] for i in range(n))
    for i, s in enumerate(starts):
        assert 0 <= s and s + T_ <= L                                        # every tile lies inside the image
        assert s <= b[i] and b[i + 1] <= s + T_                               # and holds what it owns
        for p in range(b[i], b[i + 1]):
            # P pixels of the tile on either side of an owned pixel, except towards an image border the tile touches
            assert p - s >= P or s == 0
            assert s + T_ - 1 - p >= P or s + T_ == L
    # the same numbers as the independent statement
    r_starts, r_len, owner = TR.axis(L, T_, P)
    assert (r_starts, r_len) == (starts, length)
    assert owner == [i for i in range(n) for _ in range(b[i], b[i + 1])]


def test_plan_is_the_product_of_its_axes(T):
    p = T.plan(45, 59, 3, 24, 8)
    ys, th, by = T.axis_plan(45, 24, 8)
    xs, tw, bx = T.axis_plan(59, 24, 8)
    assert (p.th, p.tw, len(p.tiles)) == (24, 24, len(ys) * len(xs)) == (24, 24, 24)
    cover = torch.zeros(45 * 3, 59 * 3, dtype=torch.int32)
    for t in p.tiles:
        r0, r1, c0, c1 = p.owned_hr(t)
        cover[r0:r1, c0:c1] += 1
        assert t.y0 in ys and t.x0 in xs
    assert bool((cover == 1).all())
    one = T.plan(20, 59, 2, 0, 0)                           # tile == 0: the whole image is the one tile
    assert (one.th, one.tw, len(one.tiles)) == (20, 59, 1)
    short = T.plan(20, 59, 2, 24, 8)                        # an axis shorter than the tile
    assert (short.th, short.tw) == (20, 24)


def _conv_stack(c, scale, seed):
    """A random small x`scale` network in float64: 3x3 conv, tanh, 3x3 conv to c * scale^2 channels, pixel shuffle, 3x3 conv."""
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn(8, c, 3, 3, generator=g, dtype=torch.float64) * 0.3, torch.randn(c * scale * scale, 8, 3, 3, generator=g, dtype=torch.float64) * 0.2,
         torch.randn(c, c, 3, 3, generator=g, dtype=torch.float64) * 0.3]
    b = [torch.randn(t.shape[0], generator=g, dtype=torch.float64) * 0.1 for t in w]

    def f(x):
        y = torch.tanh(F.conv2d(x, w[0], b[0], padding=1))
        y = F.pixel_shuffle(F.conv2d(y, w[1], b[1], padding=1), scale)
        return F.conv2d(y, w[2], b[2], padding=1)
    return f


@pytest.mark.parametrize("h,w,scale,tile,pad,batch,ens", [
    (45, 59, 2, 24, 8, 5, False), (20, 59, 3, 24, 8, 4, True), (45, 59, 4, 24, 0, 1, True), (31, 17, 2, 8, 2, 64, True),
    (25, 24, 2, 24, 8, 3, False), (19, 23, 3, 0, 0, 2, True)])
def test_torch_path_matches_the_independent_statement(T, h, w, scale, tile, pad, batch, ens):
    f = _conv_stack(2, scale, seed=h * w)
    x = torch.rand(1, 2, h, w, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got = T.tiled_forward(f, x, scale, tile=tile, pad=pad, tile_batch=batch, self_ensemble=ens)
    want = TR.forward(f, x, scale, tile, pad, ens)
    assert got.dtype == torch.float64 and got.shape == want.shape and got.is_contiguous()
    # float64 round-off: the two differ only in the batch size f sees and in the grouping of the eight-term sum
    tol = 64 * EPS64 * max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"TILING torch path vs statement: max |diff| {err:.3e} (< {tol:.3e})")
    assert err < tol
    xs = torch.cat([x, x.flip(-1)])                          # a batch: image by image
    both = T.tiled_forward(f, xs, scale, tile=tile, pad=pad, tile_batch=batch, self_ensemble=ens)
    assert torch.equal(both[0:1], got) and both.shape[0] == 2


_EDSR_KW = dict(n_feats=64, n_resblocks=2, res_scale=0.1)     # the small EDSR of eval_ref (OVERFLOW's, without the rescaling)


def _small_edsr(scale):
    import sr_amd
    torch.manual_seed(0)
    m = sr_amd.EDSR(scale_factor=scale, **_EDSR_KW)
    sd = {k: v.detach().double() if v.is_floating_point() else v.clone() for k, v in m.state_dict().items()}

    def f(x):
        with torch.no_grad():
            return OF.forward("EDSR", sd, x.double(), scale_factor=scale, **_EDSR_KW)
    return f


def _receptive_radius(f, scale, c=3, n=27):
    """LR pixels to either side of an output pixel that f reads: an impulse at the centre LR pixel, through f, and the farthest HR
    pixel it moves, in LR pixels (HR row Y belongs to LR row Y // scale)."""
    x = torch.full((1, c, n, n), 0.5, dtype=torch.float64)
    x2 = x.clone()
    x2[:, :, n // 2, n // 2] += 0.25
    moved = ((f(x2) - f(x)).abs().amax(dim=(0, 1)) > 0).nonzero()
    r = int(((moved // scale) - n // 2).abs().max())
    assert r < n // 2 - 1, "the probe image is too small for this network"
    return r


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_tiled_equals_whole_when_the_pad_covers_the_receptive_radius(T, scale):
    f = _small_edsr(scale)
    tile, pad = 24, 8
    radius = _receptive_radius(f, scale)
    print(f"TILING small EDSR x{scale}: receptive radius {radius} LR pixels, pad {pad}")
    assert pad >= radius
    x = torch.rand(1, 3, 45, 59, generator=torch.Generator().manual_seed(scale), dtype=torch.float64)
    whole = f(x)
    scale_of = max(1.0, float(whole.abs().max()))
    for fwd in (lambda p: T.tiled_forward(f, x, scale, tile=tile, pad=p, tile_batch=5), lambda p: TR.forward(f, x, scale, tile, p)):
        err = float((fwd(pad) - whole).abs().max())
        # float64 round-off of ~10 layers of 576-term sums taken in another order (another image size)
        assert err < 1e4 * EPS64 * scale_of, err
        seam = float((fwd(0) - whole).abs().max())
        print(f"TILING small EDSR x{scale}: |tiled - whole| pad {pad}: {err:.3e}, pad 0: {seam:.3e}")
        assert seam > 1e-6 * scale_of, "pad 0 shows no seam: the test cannot see one"


@pytest.mark.parametrize("k", range(8))
def test_transforms_invert(T, k):
    x = torch.rand(2, 3, 5, 7, generator=torch.Generator().manual_seed(k))
    for mod in (T, TR):
        t = mod.transform(x, k)
        assert tuple(t.shape[-2:]) == ((7, 5) if k & 4 else (5, 7))
        assert torch.equal(mod.inverse(t, k), x)
    assert torch.equal(T.transform(x, k), TR.transform(x, k))
    # bit 0 reverses W, bit 1 reverses H, bit 2 transposes after the flips
    Y, X = 1, 2
    y1, x1 = (X, Y) if k & 4 else (Y, X)
    y, xx = (4 - y1 if k & 2 else y1), (6 - x1 if k & 1 else x1)
    assert torch.equal(T.transform(x, k)[:, :, Y, X], x[:, :, y, xx])


def test_ensemble_of_an_equivariant_map_is_the_map(T):
    """f commutes with the 8 transforms (a kernel symmetric under them, a pointwise nonlinearity, nearest upsampling)."""
    a, b, c = 0.5, 0.125, -0.0625
    k = torch.tensor([[c, b, c], [b, a, b], [c, b, c]], dtype=torch.float64).view(1, 1, 3, 3).repeat(2, 1, 1, 1)

    def f(x):
        return F.interpolate(torch.tanh(F.conv2d(x, k, padding=1, groups=2)), scale_factor=2, mode="nearest")
    x = torch.rand(1, 2, 13, 21, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    want = f(x)
    for got in (T.tiled_forward(f, x, 2, self_ensemble=True), TR.forward(f, x, 2, self_ensemble=True),
                T.tiled_forward(f, x, 2, tile=8, pad=1, tile_batch=3, self_ensemble=True)):
        assert float((got - want).abs().max()) < 16 * EPS64


def test_argument_validation(T):
    import sr_amd
    for bad in (dict(tile=16, tile_pad=8), dict(tile=-1), dict(tile=24, tile_pad=-1), dict(tile=24, tile_pad=8, tile_batch=0),
                dict(tile=24, tile_pad=8, tile_batch=-3), dict(tile=24.0, tile_pad=8), dict(tile=24)):     # the default pad needs a larger tile
        with pytest.raises(ValueError):
            sr_amd.SRCNN(**bad)
        with pytest.raises(ValueError):
            T.check_args(bad.get("tile", 0), bad.get("tile_pad", T.DEFAULT_TILE_PAD), bad.get("tile_batch", T.DEFAULT_TILE_BATCH))
    m = sr_amd.SRCNN()
    assert (m._tile, m._self_ensemble) == (0, False)                 # off by default
    m = sr_amd.SRCNN(tile=24, tile_pad=8, tile_batch=5, self_ensemble=True)
    assert (m._tile, m._tile_pad, m._tile_batch, m._self_ensemble) == (24, 8, 5, True)
    assert sr_amd.SRCNN(self_ensemble=True)._tile == 0               # the ensemble alone needs no tile
    with pytest.raises(ValueError):
        T.tiled_forward(lambda t: t, torch.rand(1, 1, 4, 4), 1, tile=4, pad=2)
    with pytest.raises(ValueError):                                  # fn must return scale x the tile
        T.tiled_forward(lambda t: t, torch.rand(1, 1, 4, 4), 2, tile=3, pad=1)


def test_off_is_the_whole_image_path_on_cpu():
    import sr_amd
    torch.manual_seed(0)
    m = sr_amd.SRCNN(scale_factor=2).eval()
    x = torch.rand(1, 3, 12, 15)
    with torch.no_grad():
        assert torch.equal(m._eval_forward(x), m(x))
        assert torch.equal(m.predict_step({"lr": x}, 0), m(x).clamp(0, 1))


def test_predict_cli_tiled_self_ensemble_on_cpu(tmp_path):
    """predict.py --tile ... --self_ensemble with SRCNN on the CPU: the PNG is the independent statement around the model's float64
    twin, through SRModel.to_uint8.  The fp32 run may differ from float64 by far less than `margin` grey levels; the input is one
    whose float64 image keeps that distance from every rounding boundary, so the two round alike."""
    import sr_amd
    from PIL import Image
    import predict
    scale, tile, pad = 2, 8, 2
    torch.manual_seed(0)
    m = sr_amd.SRCNN(scale_factor=scale).eval()
    ckpt = tmp_path / "srcnn.pt"
    torch.save(m.state_dict(), ckpt)
    m64 = copy.deepcopy(m).double()

    def f(x):
        with torch.no_grad():
            return m64(x)
    margin = 1e-3
    for seed in range(20):
        x = torch.rand(3, 13, 17, generator=torch.Generator().manual_seed(seed))
        want = TR.forward(f, x[None], scale, tile, pad, True)[0]
        v = want.clamp(0, 1) * 255.0 + 0.5
        if float(((v - v.round()).abs())[(want > 0) & (want < 1)].min()) > margin and float(want.abs().min()) * 255 > margin \
                and float((want - 1).abs().min()) * 255 > margin:
            break
    else:
        pytest.fail("no seed keeps the reference image off the rounding boundaries")
    assert float(((want > 0) & (want < 1)).double().mean()) > 0.3, "the reference image is mostly clamped"
    d = tmp_path / "SetT"
    d.mkdir()
    np.save(d / "img.npy", x.numpy())
    out = tmp_path / "out"
    predict.main(["-m", "srcnn", "-s", str(scale), "--checkpoint", str(ckpt), "--precision", "32", "--accelerator", "cpu",
                  "--default_root_dir", str(out), "--predict_datasets", str(d), "--tile", str(tile), "--tile_pad", str(pad),
                  "--tile_batch", "3", "--self_ensemble"])
    png = torch.from_numpy(np.asarray(Image.open(out / "SetT" / "img.png"))).permute(2, 0, 1)
    assert tuple(png.shape) == (3, 13 * scale, 17 * scale)
    assert torch.equal(png, sr_amd.SRModel.to_uint8(want.float())) and torch.equal(png, sr_amd.SRModel.to_uint8(want))
    # and the flags reach the model: without them the image is another one
    predict.main(["-m", "srcnn", "-s", str(scale), "--checkpoint", str(ckpt), "--precision", "32", "--accelerator", "cpu",
                  "--default_root_dir", str(tmp_path / "plain"), "--predict_datasets", str(d)])
    plain = torch.from_numpy(np.asarray(Image.open(tmp_path / "plain" / "SetT" / "img.png"))).permute(2, 0, 1)
    assert not torch.equal(plain, png)


def test_header_and_binding_agree_on_the_tile_structs():
    """The two structs of csrc/tile.hip are the header's (tests/test_host_surface.py checks every struct's layout against the C
    compiler's, and that the entry points are declared, bound and exported)."""
    import sr_amd as A
    assert A._lib.STRUCTS["srk_tile_desc"] is A._lib.TileDesc and A._lib.STRUCTS["srk_tile_args"] is A._lib.TileArgs
    assert A._lib.LAUNCHERS["srk_tile_gather"] is A._lib.LAUNCHERS["srk_tile_place"] is A._lib.TileArgs
