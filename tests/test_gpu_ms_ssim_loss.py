"""MS-SSIM loss on the MI355X (csrc/ms_ssim_loss.hip through sr_amd.ms_ssim_loss): the HIP loss and gradient against the float64
statement of tests/ms_ssim_loss_ref.py, many planes, determinism, the upstream gradient, the tie to the shipped metric, the plane
whose value is 0, the torch fallbacks, the refusals and the graphed training step."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ms_ssim_loss_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(sr, hr, float64 loss, float64 gradient) of one shape: computed once, read by every test that needs it."""
    sr, hr = REF.images(shape, 11 + sum(shape))
    return (sr, hr) + REF.loss_and_grad(sr, hr)


def _hip_loss_grad(A, sr, hr, weight=1.0):
    s = sr.detach().cuda().float().contiguous().requires_grad_(True)
    loss = A.ops.MSSSIMLossFn.apply(s, hr.cuda().float().contiguous())
    (weight * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), s.grad.detach()


# The limits (REF.LIMIT_*: |d loss| 1e-5, relative L2 1e-3, max 3e-3 of the largest entry) are at least three times what the plain
# fp32 torch statement costs on these inputs (tests/test_ms_ssim_loss_cpu.py measures that: 2.4e-7, 1.1e-5, 4.0e-5) and are the SSIM
# loss's own; the margin is for the kernel's summation order.  The map tile is 16 x 16 positions and the backward tile 16 x 32 pixels
# of a level: 161 has a single map position at level 4 and every level odd (p = 1 everywhere), 176 no padding at all, 162 x 161 and
# 161 x 176 drop a padded row / column, 163 x 209 mixes the parities down the levels, 192 has several tiles on levels 0 to 2.
@pytest.mark.parametrize("shape", REF.SHAPES, ids=["x".join(map(str, s)) for s in REF.SHAPES])
def test_hip_matches_float64(A, shape):
    sr, hr, l64, g64 = _case(shape)
    loss, g = _hip_loss_grad(A, sr, hr)
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    print(f"\n{shape}: loss {float(loss):.6f}, |dloss| {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert torch.isfinite(g).all()
    assert dl <= REF.LIMIT_LOSS
    assert l2 <= REF.LIMIT_L2
    assert worst <= REF.LIMIT_MAX
    outside = (sr < 0) | (sr > 1)
    assert outside.any() and float(g.cpu()[outside].abs().max()) == 0.0


def test_more_blocks_than_a_16_bit_grid_dimension(A):
    """(256, 3, 161, 161): 768 planes.  Every launch carries (plane, tile) in blockIdx.x, the one grid dimension that is not limited
    to 65535 blocks; with blockIdx.y for the planes (the metric's layout) N * C would end at 65535, and the smallest batch that
    shows it, (21846, 3, 161, 161), is 1.7 G pixels.  What can wrap at this size is the flat index itself: the maps launch has
    768 * 131 = 100608 blocks, the level-0 backward 768 * 66 = 50688 and the pooling 768 * 26, so a 16-bit block index, or a plane
    taken from the wrong dimension, mixes planes up from plane 500 on.  The images are A, B, A, B, ..., A, C (the last image is
    unlike every other), so the float64 statement is needed for three images only: image i's gradient is its own one-image
    gradient over 256, and the loss is the mean of the per-image losses."""
    n = 256
    sr3, hr3 = REF.images((3, 3, 161, 161), 7)
    ref = [REF.loss_and_grad(sr3[i:i + 1], hr3[i:i + 1]) for i in range(3)]
    order = [0, 1] * (n // 2 - 1) + [0, 2]
    idx = torch.tensor(order)
    loss, g = _hip_loss_grad(A, sr3[idx], hr3[idx])
    l64 = sum(float(ref[i][0]) for i in order) / n
    assert g.shape == (n, 3, 161, 161)
    assert abs(float(loss) - l64) <= REF.LIMIT_LOSS
    for pos in (0, 1, n // 2, n // 2 + 1, n - 2, n - 1):               # the first, the middle and the last images, the last separately
        want = ref[order[pos]][1][0] / n
        got = g[pos].cpu().double()
        l2 = float((got - want).norm() / want.norm())
        worst = float((got - want).abs().max() / want.abs().max())
        print(f"\nimage {pos}: grad rel L2 {l2:.2e}, max {worst:.2e}")
        assert l2 <= REF.LIMIT_L2 and worst <= REF.LIMIT_MAX, pos
    # every copy of A (and of B) got the same bits: no plane read another plane's tiles or table row
    assert torch.equal(g[0::2][:-1], g[0:1].expand(n // 2 - 1, -1, -1, -1)) and torch.equal(g[0], g[n - 2])
    assert torch.equal(g[1::2][:-1], g[1:2].expand(n // 2 - 1, -1, -1, -1))
    last = (g[-1].cpu().double() - ref[2][1][0] / n).abs().max() / (ref[2][1][0] / n).abs().max()
    assert float(last) <= REF.LIMIT_MAX, "the last plane got its own gradient"


def test_deterministic(A):
    sr, hr = REF.images((2, 3, 163, 209), 3)
    l1, g1 = _hip_loss_grad(A, sr, hr)
    l2, g2 = _hip_loss_grad(A, sr, hr)
    assert float(l1) == float(l2) and torch.equal(g1, g2), "fixed-order reductions and a gather-form backward: bit-identical runs"


def test_upstream_gradient(A):
    sr, hr = REF.images((2, 3, 162, 161), 4)
    l1, g1 = _hip_loss_grad(A, sr, hr)
    l3, g3 = _hip_loss_grad(A, sr, hr, weight=3.5)
    assert float(l3) == float(l1)
    assert float(g1.abs().max()) > 0.0
    assert torch.allclose(g3, 3.5 * g1, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("shape", [(2, 3, 161, 176), (1, 2, 192, 192)], ids=["161x176", "192"])
def test_loss_is_one_minus_the_shipped_metric(A, shape):
    sr, hr = REF.images(shape, 5, spill=False)
    x, y = sr.clamp(0, 1).cuda(), hr.cuda()
    loss = A.ops.ms_ssim_loss(x, y)
    assert loss.dim() == 0 and loss.is_cuda
    assert abs(float(loss) - (1.0 - float(A.ops.ms_ssim(x, y)))) <= 1e-5


def test_anticorrelated_plane_gets_a_zero_gradient(A):
    """Plane (0, 0) has sr = 1 - hr: its level means are negative (checked in float64 in tests/test_ms_ssim_loss_cpu.py), its value
    is 0 and, unlike piq's NaN, its gradient is exactly 0; the other planes of the image keep theirs."""
    sr, hr = REF.anticorrelated(0)
    l64, g64 = REF.loss_and_grad(sr, hr)
    loss, g = _hip_loss_grad(A, sr, hr)
    assert torch.isfinite(g).all()
    assert float(g[0, 0].abs().max()) == 0.0
    assert float(g[0, 1].abs().max()) > 0.0 and float(g[0, 2].abs().max()) > 0.0
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    print(f"\n|dloss| {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert dl <= REF.LIMIT_LOSS and l2 <= REF.LIMIT_L2 and worst <= REF.LIMIT_MAX


def test_fallbacks_take_the_torch_path(A, monkeypatch):
    calls = []
    real = A.ops.MSSSIMLossFn.apply
    monkeypatch.setattr(A.ops.MSSSIMLossFn, "apply", lambda *a: calls.append(1) or real(*a))
    from sr_amd import ms_ssim_loss as ML
    sr, hr, l64, _ = _case((1, 1, 161, 161))
    s, h = sr.cuda(), hr.cuda()
    want = float(l64)
    # hr needing a gradient, float64 inputs and strided views go to ms_ssim_torch
    hg = h.clone().requires_grad_(True)
    assert abs(float(ML.ms_ssim_loss(s, hg).detach()) - want) <= 1e-5
    assert abs(float(ML.ms_ssim_loss(s.double(), h.double())) - want) <= 1e-10
    wide_s, wide_h = torch.zeros(1, 1, 161, 168, device="cuda"), torch.zeros(1, 1, 161, 168, device="cuda")
    wide_s[..., :161], wide_h[..., :161] = s, h
    vs, vh = wide_s[..., :161], wide_h[..., :161]
    assert not vs.is_contiguous()
    assert abs(float(ML.ms_ssim_loss(vs, vh)) - want) <= 1e-5
    assert abs(float(ML.ms_ssim_loss(s, vh)) - want) <= 1e-5
    assert calls == []
    assert abs(float(ML.ms_ssim_loss(s, h)) - want) <= 1e-5
    assert calls == [1]


def test_refusals_on_the_gpu(A):
    for hw in ((160, 192), (192, 160)):
        x = torch.rand(1, 3, *hw, device="cuda")
        with pytest.raises(ValueError):
            A.ops.ms_ssim_loss(x, x)
        with pytest.raises(ValueError):
            A.ops.MSSSIMLossFn.apply(x, x)
    with pytest.raises(ValueError):
        A.ops.ms_ssim_loss(torch.rand(1, 3, 161, 161, device="cuda"), torch.rand(1, 3, 161, 162, device="cuda"))
    with pytest.raises(ValueError):
        A.ops.MSSSIMLossFn.apply(torch.rand(1, 3, 161, 161, device="cuda"), torch.rand(1, 3, 161, 162, device="cuda"))


def _fit(A, use_graph):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=4, precision=32, n_feats=32, n_resblocks=2, res_scale=0.1, losses="0.16*l1+0.84*ms_ssim", patch_size=176)
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(4, 3, 44, 4, 400 + i, "cpu") for i in range(8)))
    torch.cuda.synchronize()
    return tr, [p.detach().clone() for p in m.parameters()]


def test_graphed_step_with_ms_ssim_follows_the_eager_loop(A):
    (tg, pg), (te, pe) = _fit(A, True), _fit(A, False)
    g = tg.graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step with the MS-SSIM loss was captured"
    lg, le = tg.losses, te.losses
    assert len(lg) == len(le) == 8 and all(np.isfinite(lg))
    # every launch of the step sums in a fixed order ("Reproducibility"): the replayed step gives the eager loop's bits
    assert np.array_equal(np.asarray(lg, np.float32).view(np.int32), np.asarray(le, np.float32).view(np.int32)), (lg, le)
    for a, b in zip(pg, pe):
        assert torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), float((a - b).abs().max())
