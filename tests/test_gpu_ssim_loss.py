"""SSIM loss on the MI355X (csrc/ssim_loss.hip through sr_amd.ssim_loss): the HIP loss and gradient against the float64 statement
of tests/ssim_loss_ref.py, many planes, determinism, the upstream gradient, the tie to the shipped metric, the torch fallbacks and
the graphed training step."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_loss_ref as REF  # noqa: E402

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
    loss = A.ops.SSIMLossFn.apply(s, hr.cuda().float().contiguous())
    (weight * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), s.grad.detach()


# The limits (REF.LIMIT_*: |d loss| 1e-5, relative L2 1e-3, max 3e-3 of the largest entry) are at least three times what the plain
# fp32 torch statement costs on these inputs (tests/test_ssim_loss_cpu.py measures that: 6.3e-7, 2.8e-5, 3.8e-5) and no looser than
# HaarPSI's; the margin is for the kernel's summation order.  The forward tile is 16 x 16 map positions: 26 x 26 is one tile exactly,
# 27 x 27 one more each way; the backward tile is 16 x 32 pixels, which 27 x 38 and 33 x 33 cross both ways.
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


def test_more_planes_than_a_grid_dimension(A):
    """N * C = 65538 planes of one map position each: (plane, tile) share one grid dimension, so nothing wraps at 65535."""
    shape = (21846, 3, 11, 11)
    sr, hr = REF.images(shape, 7)
    l64, g64 = REF.loss_and_grad(sr, hr)
    loss, g = _hip_loss_grad(A, sr, hr)
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    print(f"\n{shape}: |dloss| {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert dl <= REF.LIMIT_LOSS and l2 <= REF.LIMIT_L2 and worst <= REF.LIMIT_MAX
    last = (g[-1].cpu().double() - g64[-1]).abs().max() / g64[-1].abs().max()
    assert float(last) <= REF.LIMIT_MAX, "the last plane got its own gradient"


def test_deterministic(A):
    sr, hr = REF.images((4, 3, 96, 80), 3)
    l1, g1 = _hip_loss_grad(A, sr, hr)
    l2, g2 = _hip_loss_grad(A, sr, hr)
    assert float(l1) == float(l2) and torch.equal(g1, g2), "fixed-order reductions: bit-identical runs"


def test_upstream_gradient(A):
    sr, hr = REF.images((2, 3, 64, 72), 4)
    l1, g1 = _hip_loss_grad(A, sr, hr)
    l3, g3 = _hip_loss_grad(A, sr, hr, weight=3.5)
    assert float(l3) == float(l1)
    assert float(g1.abs().max()) > 0.0
    assert torch.allclose(g3, 3.5 * g1, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("shape", [(3, 3, 48, 40), (1, 2, 384, 391)], ids=["f1", "f2"])
def test_loss_is_one_minus_the_shipped_metric(A, shape):
    sr, hr = REF.images(shape, 5, spill=False)
    x, y = sr.clamp(0, 1).cuda(), hr.cuda()
    loss = A.ops.ssim_loss(x, y)
    assert loss.dim() == 0 and loss.is_cuda
    assert abs(float(loss) - (1.0 - float(A.ops.ssim(x, y)))) <= 1e-5


def test_fallbacks_take_the_torch_path(A, monkeypatch):
    calls = []
    real = A.ops.SSIMLossFn.apply
    monkeypatch.setattr(A.ops.SSIMLossFn, "apply", lambda *a: calls.append(1) or real(*a))
    from sr_amd import ssim_loss as SL
    sr, hr = REF.images((2, 3, 32, 32), 6)
    s, h = sr.cuda(), hr.cuda()
    want = float(REF.ssim_loss(sr, hr))
    # hr needing a gradient, float64 inputs and strided views go to ssim_torch
    hg = h.clone().requires_grad_(True)
    assert abs(float(SL.ssim_loss(s, hg).detach()) - want) <= 1e-5
    assert abs(float(SL.ssim_loss(s.double(), h.double())) - want) <= 1e-10
    wide_s, wide_h = torch.zeros(2, 3, 32, 40, device="cuda"), torch.zeros(2, 3, 32, 40, device="cuda")
    wide_s[..., :32], wide_h[..., :32] = s, h
    vs, vh = wide_s[..., :32], wide_h[..., :32]
    assert not vs.is_contiguous()
    assert abs(float(SL.ssim_loss(vs, vh)) - want) <= 1e-5
    assert abs(float(SL.ssim_loss(s, vh)) - want) <= 1e-5
    assert calls == []
    assert abs(float(SL.ssim_loss(s, h)) - want) <= 1e-5
    assert calls == [1]


def test_refusals_on_the_gpu(A):
    x = torch.rand(1, 3, 10, 32, device="cuda")
    with pytest.raises(ValueError):
        A.ops.ssim_loss(x, x)
    with pytest.raises(ValueError):
        A.ops.SSIMLossFn.apply(x, x)
    with pytest.raises(ValueError):
        A.ops.ssim_loss(torch.rand(1, 3, 16, 16, device="cuda"), torch.rand(1, 3, 16, 17, device="cuda"))


def _fit(A, precision, use_graph, losses="0.16*l1+0.84*ssim"):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision=precision, n_feats=32, n_resblocks=2, res_scale=0.1, losses=losses)
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 400 + i, "cpu") for i in range(8)))
    torch.cuda.synchronize()
    return tr, [p.detach().clone() for p in m.parameters()]


def test_graphed_step_with_ssim_follows_the_eager_loop(A):
    (tg, pg), (te, pe) = _fit(A, 32, True), _fit(A, 32, False)
    g = tg.graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step with the SSIM loss was captured"
    lg, le = tg.losses, te.losses
    assert len(lg) == len(le) == 8 and all(np.isfinite(lg))
    # every launch of the step sums in a fixed order ("Reproducibility"): the replayed step gives the eager loop's bits
    assert np.array_equal(np.asarray(lg, np.float32).view(np.int32), np.asarray(le, np.float32).view(np.int32)), (lg, le)
    for a, b in zip(pg, pe):
        assert torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), float((a - b).abs().max())
