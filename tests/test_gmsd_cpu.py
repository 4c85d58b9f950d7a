"""GMSD loss and metric on the CPU: `gmsd_torch` in float64 and fp32 against the float64 statement of tests/gmsd_ref.py, the fp32
floors the GPU limits rest on, the zero cases, hand-checkable values (a step edge, the zero pad), the loss string and the metric
name, the refused inputs and the ctypes mirror of the header."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmsd_ref as REF  # noqa: E402

IDS = ["x".join(map(str, s)) for s in REF.SHAPES]


@pytest.fixture(scope="module")
def G():
    from sr_amd import gmsd
    return gmsd


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(sr, hr, float64 loss, float64 gradient) of one shape: computed once, read by every test that needs it."""
    sr, hr = REF.images(shape, 11 + sum(shape))
    return (sr, hr) + REF.loss_and_grad(sr, hr)


def _loss_grad(G, sr, hr):
    s = sr.clone().requires_grad_(True)
    loss = G.gmsd_loss(s, hr)
    loss.backward()
    return loss.detach(), s.grad


# ---- gmsd_torch against the statement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", REF.SHAPES, ids=IDS)
def test_float64_torch_path_is_the_statement(G, shape):
    sr, hr, l64, g64 = _case(shape)
    loss, g = _loss_grad(G, sr.double(), hr.double())
    assert loss.dtype == torch.float64 and torch.isfinite(g).all() and torch.isfinite(g64).all()
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    assert dl <= 1e-12 and l2 <= 1e-12 and worst <= 1e-12, (dl, l2, worst)
    if shape[0] > 1:
        assert float(g[0].abs().max()) == 0.0 and float(g64[0].abs().max()) == 0.0, "the image equal to its reference"
    if shape == (1, 1, 2, 2):
        assert float(loss) == 0.0 and float(l64) == 0.0, "one pooled position has no deviation"


@pytest.mark.parametrize("shape", REF.SHAPES, ids=IDS)
def test_fp32_torch_path_stays_within_the_limits(G, shape):
    """Measured over REF.SHAPES: |d loss| <= 5.9e-9, gradient relative L2 <= 3.1e-6, max error <= 1.1e-5 of the largest entry."""
    sr, hr, l64, g64 = _case(shape)
    loss, g = _loss_grad(G, sr, hr)
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    print(f"\n{shape}: loss {float(loss):.6f}, |dloss| {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and torch.isfinite(g).all()
    assert dl <= REF.LIMIT_LOSS and l2 <= REF.LIMIT_L2 and worst <= REF.LIMIT_MAX
    outside = (sr < 0) | (sr > 1)
    if outside.any():
        assert float(g[outside].abs().max()) == 0.0


def test_fp32_reference_statement_sets_the_limits():
    """The limits' calibration: the reference statement ITSELF in fp32 against itself in float64, on the GPU tests' inputs.  Measured
    over REF.SHAPES: |d loss| <= 2.7e-8, gradient relative L2 <= 8.2e-6, max error <= 1.1e-5 of the largest entry (REF.FLOOR_*).  The
    limits are ten times the floors (at least three are asked for), and no looser than the SSIM loss's."""
    worst = [0.0, 0.0, 0.0]
    for shape in REF.SHAPES:
        sr, hr, l64, g64 = _case(shape)
        e = REF.errors(*REF.loss_and_grad(sr, hr, torch.float32), l64, g64)
        print(f"\n{shape}: |dloss| {e[0]:.2e}, grad rel L2 {e[1]:.2e}, max {e[2]:.2e}")
        worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"\nfloors: {worst[0]:.2e} {worst[1]:.2e} {worst[2]:.2e}")
    for got, floor, limit, cap in zip(worst, (REF.FLOOR_LOSS, REF.FLOOR_L2, REF.FLOOR_MAX), (REF.LIMIT_LOSS, REF.LIMIT_L2, REF.LIMIT_MAX),
                                      (1e-5, 1e-3, 3e-3)):
        assert 3 * got <= limit, "at least a threefold margin over what fp32 costs the statement itself"
        assert 3 * floor <= limit <= cap


# ---- the zero cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_identical_and_constant_pairs_give_exact_zeros(G, dtype):
    _, hr = REF.images((2, 3, 37, 40), 31)
    flat = torch.full((2, 3, 37, 40), 0.5)
    for img in (hr.to(dtype), flat.to(dtype), flat[:, :1].to(dtype)):
        loss, g = _loss_grad(G, img, img.clone())
        assert float(loss) == 0.0
        assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0
        l64, g64 = REF.loss_and_grad(img, img)
        assert float(l64) == 0.0 and torch.isfinite(g64).all() and float(g64.abs().max()) == 0.0
        assert float(G.gmsd(img, img.clone())) == 0.0


def test_flat_regions_of_one_image_keep_the_gradient_finite(G):
    """A flat test image against a textured reference: a = 0 at every interior position (piq's autograd gives NaN there), the
    border positions see the zero padding and carry the whole gradient.  (One plane of 1/4: sums of a few such values are exact in
    any order, so the statement's dense convolution gives an exact 0 there too.)"""
    _, hr = REF.images((1, 1, 24, 28), 32)
    sr = torch.full_like(hr, 0.25)
    loss, g = _loss_grad(G, sr, hr)
    l64, g64 = REF.loss_and_grad(sr, hr)
    assert float(loss) > 0.0 and torch.isfinite(g).all() and torch.isfinite(g64).all()
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    assert dl <= REF.LIMIT_LOSS and l2 <= REF.LIMIT_L2 and worst <= REF.LIMIT_MAX
    assert float(g64[..., 6:-6, 6:-6].abs().max()) == 0.0 and float(g[..., 6:-6, 6:-6].abs().max()) == 0.0
    assert float(g64.abs().max()) > 0.0


def test_gradient_is_zero_outside_the_unit_range_and_passes_on_its_ends(G):
    sr, hr = REF.images((1, 3, 24, 24), 25)
    sr[0, 0, 12, 12], sr[0, 1, 12, 13], sr[0, 2, 13, 12] = 0.0, 1.0, 0.0          # exactly on the ends of the closed interval
    _, g = _loss_grad(G, sr, hr)
    outside = (sr < 0) | (sr > 1)
    assert outside.sum() > 100
    assert float(g[outside].abs().max()) == 0.0
    _, g64 = REF.loss_and_grad(sr, hr)
    assert float(g64[outside].abs().max()) == 0.0
    for p in ((0, 0, 12, 12), (0, 1, 12, 13), (0, 2, 13, 12)):
        assert float(g[p]) != 0.0 and float(g64[p]) != 0.0, p


# ---- hand-checkable values --------------------------------------------------------------------------------------------------------
def test_step_edge_on_a_4x4_plane_by_hand(G):
    """hr: a vertical step edge 0 | 1, sr: the same edge at half the contrast 0 | 1/2.  Pooled 2 x 2 maps Y = [[0, 1], [0, 1]] and
    X = Y / 2.  With the zero padding, at the two left positions gx = (1 + 1) / 3 and gy = +-1 / 3, so b = sqrt(5) / 3; at the two
    right positions gx = 0 (the left neighbours are 0, the right ones padding) and gy = +-1 / 3, so b = 1 / 3; a = b / 2 throughout.
    GMS = (2ab + c) / (a^2 + b^2 + c) takes two values, twice each, so its population deviation is half their distance."""
    hr = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float64).repeat(4, 1).view(1, 1, 4, 4)
    sr = hr / 2
    c = 170.0 / 255.0 ** 2
    left = (2 * (5.0 / 18.0) + c) / (5.0 / 36.0 + 5.0 / 9.0 + c)          # a = sqrt(5) / 6, b = sqrt(5) / 3
    right = (2 * (1.0 / 18.0) + c) / (1.0 / 36.0 + 1.0 / 9.0 + c)         # a = 1 / 6,       b = 1 / 3
    want = abs(left - right) / 2
    assert want > 1e-3
    assert abs(float(G.gmsd_torch(sr, hr)) - want) <= 1e-12
    assert abs(float(REF.gmsd_index(sr, hr)) - want) <= 1e-12
    assert abs(float(G.gmsd_torch(sr.float(), hr.float())) - want) <= 1e-6


@pytest.mark.parametrize("hw,pad", [((5, 4), [0, 0, 0, 1]), ((4, 5), [0, 1, 0, 0])], ids=["5x4", "4x5"])
def test_odd_sizes_take_the_zero_pad(G, hw, pad):
    """The last pooled row (5 x 4) or column (4 x 5) averages real pixels with zeros: the value is that of the image with a row /
    column of zeros appended, and not that of the image replicate-padded."""
    g = torch.Generator().manual_seed(33)
    hr = 0.25 + 0.5 * torch.rand(1, 1, *hw, generator=g, dtype=torch.float64)
    sr = (hr + 0.1 * torch.randn(1, 1, *hw, generator=g, dtype=torch.float64)).clamp(0, 1)
    got = float(G.gmsd_torch(sr, hr))
    zero = float(G.gmsd_torch(F.pad(sr, pad), F.pad(hr, pad)))
    repl = float(G.gmsd_torch(F.pad(sr, pad, mode="replicate"), F.pad(hr, pad, mode="replicate")))
    assert abs(got - zero) <= 1e-12
    assert abs(got - repl) >= 1e-5, (got, repl)
    assert abs(float(REF.gmsd_index(sr, hr)) - zero) <= 1e-12
    assert abs(float(REF.gmsd_index(sr, hr)) - float(REF.gmsd_index(F.pad(sr, pad, mode="replicate"), F.pad(hr, pad, mode="replicate")))) >= 1e-5


# ---- the loss string and the metric name --------------------------------------------------------------------------------------------
def test_model_accepts_gmsd_loss_and_metric():
    import sr_amd
    for losses in ("gmsd", "0.9*l1+0.1*gmsd", "l1 + 0.5*GMSD"):
        m = sr_amd.SRCNN(scale_factor=2, losses=losses, metrics=["GMSD"])
        assert "gmsd" in [l.name for l in m._losses]
        assert [n for n, _ in m._metrics] == ["GMSD"]
    m = sr_amd.SRCNN(scale_factor=2, losses="0.9*l1+0.1*gmsd")
    assert [(l.name, l.weight) for l in m._losses] == [("l1", 0.9), ("gmsd", 0.1)]
    g = torch.Generator().manual_seed(0)
    lr, hr = torch.rand(2, 3, 12, 12, generator=g), torch.rand(2, 3, 24, 24, generator=g)
    out = m.training_step({"lr": lr, "hr": hr}, 0)
    assert set(out) == {"loss", "loss/l1", "loss/gmsd"}
    out["loss"].backward()
    sr = m(lr).detach()
    want = 0.9 * float(F.l1_loss(sr.double(), hr.double())) + 0.1 * float(REF.gmsd_loss(sr, hr))
    assert abs(float(out["loss"].detach()) - want) <= 1e-6
    assert abs(float(out["loss/gmsd"].detach()) - 0.1 * float(REF.gmsd_loss(sr, hr))) <= 1e-6, "the weighted term, as the other losses log it"
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    solo = sr_amd.SRCNN(scale_factor=2, losses="gmsd").training_step({"lr": lr, "hr": hr}, 0)
    assert set(solo) == {"loss", "loss/gmsd"}
    m2 = sr_amd.SRCNN(scale_factor=2, metrics=["PSNR", "GMSD"], eval_datasets=["X"])
    res = m2.validation_step({"lr": lr, "hr": hr}, 0)
    assert set(res) == {"X/PSNR", "X/GMSD"}
    assert res["X/GMSD"].grad_fn is None
    assert abs(float(res["X/GMSD"]) - float(REF.gmsd_index(m2(lr).detach().clamp(0, 1), hr))) <= 1e-6
    gray = sr_amd.SRCNN(scale_factor=2, channels=1, losses="gmsd", metrics=["GMSD"])
    assert set(gray.training_step({"lr": lr[:, :1], "hr": hr[:, :1]}, 0)) == {"loss", "loss/gmsd"}


def test_edge_loss_stays_out_of_scope():
    import sr_amd
    with pytest.raises(NotImplementedError):
        sr_amd.SRCNN(scale_factor=2, losses="edge_loss")
    with pytest.raises(NotImplementedError):
        sr_amd.SRCNN(scale_factor=2, losses="0.9*l1+0.1*edge_loss")


def test_ops_reexports():
    import sr_amd
    for name in ("gmsd_torch", "GMSDLossFn", "gmsd_loss", "gmsd"):
        assert hasattr(sr_amd.ops, name), name


# ---- refused inputs ---------------------------------------------------------------------------------------------------------------
def test_two_channels_and_mismatched_shapes_raise(G):
    x = torch.rand(1, 2, 8, 8)
    for fn in (G.gmsd_torch, G.gmsd_loss, G.gmsd):
        with pytest.raises(ValueError):
            fn(x, x)
        with pytest.raises(ValueError):
            fn(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17))
        with pytest.raises(ValueError):
            fn(torch.rand(3, 16, 16), torch.rand(3, 16, 16))
    with pytest.raises(ValueError):
        REF.gmsd_index(x, x)


def test_the_metric_carries_no_gradient_and_is_the_loss_value(G):
    sr, hr = REF.images((2, 3, 20, 22), 34)
    s = sr.clone().requires_grad_(True)
    v = G.gmsd(s, hr)
    assert v.grad_fn is None and not v.requires_grad
    assert float(v) == float(G.gmsd_loss(sr, hr))


def test_hip_entry_refuses_the_cpu(G):
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError):
        G.GMSDLossFn.apply(x, x)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_gmsd_args_mirror_the_header():
    import sr_amd
    assert sr_amd._lib.STRUCTS["srk_gmsd_args"] is sr_amd._lib.GmsdArgs       # its layout: tests/test_host_surface.py
    assert all(sr_amd._lib.LAUNCHERS["srk_gmsd_" + k] is sr_amd._lib.GmsdArgs for k in ("fwd", "finalize", "bwd"))
    assert "srk_gmsd_tiles" in sr_amd._lib.OTHER_SYMBOLS


def test_tile_count_and_refusals_of_the_library():
    """srk_gmsd_tiles is host code: the pooled map ((H + p) // 2 x (W + p) // 2) is tiled 16 x 32 per image, and what cannot run is
    refused with -1."""
    import sr_amd
    tiles = sr_amd._lib.load().srk_gmsd_tiles
    assert tiles(1, 1, 2, 2) == 1 and tiles(1, 3, 5, 4) == 1 and tiles(1, 1, 32, 64) == 1
    assert tiles(1, 3, 34, 66) == 4 and tiles(1, 3, 33, 64) == 2 and tiles(1, 3, 32, 65) == 2
    assert tiles(2, 1, 37, 71) == 2 * 4 and tiles(16, 3, 192, 192) == 16 * 6 * 3 and tiles(1, 3, 203, 331) == 7 * 6
    assert tiles(65538, 1, 4, 4) == 65538
    assert tiles(1, 2, 8, 8) == -1 and tiles(1, 4, 8, 8) == -1 and tiles(0, 3, 8, 8) == -1 and tiles(1, 3, 0, 8) == -1
    assert tiles(1 << 27, 3, 192, 192) == -1                # images x tiles past 2^31
