"""GMSD loss and metric on the MI355X (csrc/gmsd.hip through sr_amd.gmsd): the HIP loss and gradient against the float64 statement of
tests/gmsd_ref.py, more images than a grid dimension, determinism, the upstream gradient, the metric, the torch fallbacks, the
refusals and the graphed training step."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmsd_ref as REF  # noqa: E402

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
    loss = A.ops.GMSDLossFn.apply(s, hr.cuda().float().contiguous())
    (weight * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), s.grad.detach()


# The limits (REF.LIMIT_*: |d loss| 2.7e-7, relative L2 8.2e-5, max 1.1e-4 of the largest entry) are ten times what the float64
# statement itself costs when it runs in fp32 on these inputs (tests/test_gmsd_cpu.py measures that: 2.7e-8, 8.2e-6, 1.1e-5), and
# tighter than the SSIM loss's; the margin is for the kernel's summation order, square root and division.  Forward and backward
# tile the pooled map 16 x 32 (32 x 64 pixels of sr): 32 x 64 is one tile exactly, 34 x 66 one position more each way, 37 x 71
# crosses the tile both ways with odd sizes (the pad row and column), 203 x 331 has 7 x 6 tiles with both edges partial and padded.
# Even widths take the 8-byte loads and stores, odd widths the scalar ones.
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
    assert outside.any() or min(shape[2:]) < 4, "every shape but the smallest has pixels outside [0, 1]"
    if outside.any():
        assert float(g.cpu()[outside].abs().max()) == 0.0
    if shape[0] > 1:
        assert float(g[0].abs().max()) == 0.0, "the image equal to its reference has zero variance and gets no gradient"
        assert float(g[1:].abs().max()) > 0.0
    if shape == (1, 1, 2, 2):
        assert float(loss) == 0.0 and float(g.abs().max()) == 0.0, "one pooled position has no deviation"


def test_more_images_than_a_grid_dimension(A):
    """65538 images of 2 x 2 map positions each: (image, tile) share one grid dimension, so nothing wraps at 65535."""
    shape = (65538, 1, 4, 4)
    sr, hr = REF.images(shape, 7)
    l64, g64 = REF.loss_and_grad(sr, hr)
    loss, g = _hip_loss_grad(A, sr, hr)
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    print(f"\n{shape}: |dloss| {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert dl <= REF.LIMIT_LOSS and l2 <= REF.LIMIT_L2 and worst <= REF.LIMIT_MAX
    assert float(g64[-1].abs().max()) > 0.0
    last = (g[-1].cpu().double() - g64[-1]).abs().max() / g64[-1].abs().max()
    assert float(last) <= REF.LIMIT_MAX, "the last image got its own gradient"
    assert float(g[0].abs().max()) == 0.0


def test_deterministic(A):
    sr, hr = REF.images((4, 3, 96, 81), 3)
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


@pytest.mark.parametrize("shape", [(3, 3, 48, 40), (2, 1, 37, 71)], ids=["rgb", "gray-odd"])
def test_metric_is_the_loss_value_without_a_gradient(A, shape):
    sr, hr = REF.images(shape, 5, spill=False)
    x, y = sr.clamp(0, 1).cuda().requires_grad_(True), hr.cuda()
    m = A.ops.gmsd(x, y)
    assert m.dim() == 0 and m.is_cuda and m.grad_fn is None and not m.requires_grad
    assert abs(float(m) - float(A.ops.gmsd_loss(x, y).detach())) <= 1e-6
    assert abs(float(m) - float(REF.gmsd_index(sr.clamp(0, 1), hr))) <= 1e-6


def test_fallbacks_take_the_torch_path(A, monkeypatch):
    calls = []
    real = A.ops.GMSDLossFn.apply
    monkeypatch.setattr(A.ops.GMSDLossFn, "apply", lambda *a: calls.append(1) or real(*a))
    from sr_amd import gmsd as GM
    sr, hr = REF.images((2, 3, 32, 32), 6)
    s, h = sr.cuda(), hr.cuda()
    want = float(REF.gmsd_loss(sr, hr))
    # hr needing a gradient, float64 inputs and strided views go to gmsd_torch
    hg = h.clone().requires_grad_(True)
    assert abs(float(GM.gmsd_loss(s, hg).detach()) - want) <= 1e-6
    assert abs(float(GM.gmsd_loss(s.double(), h.double())) - want) <= 1e-10
    wide_s, wide_h = torch.zeros(2, 3, 32, 40, device="cuda"), torch.zeros(2, 3, 32, 40, device="cuda")
    wide_s[..., :32], wide_h[..., :32] = s, h
    vs, vh = wide_s[..., :32], wide_h[..., :32]
    assert not vs.is_contiguous()
    assert abs(float(GM.gmsd_loss(vs, vh)) - want) <= 1e-6
    assert abs(float(GM.gmsd_loss(s, vh)) - want) <= 1e-6
    assert abs(float(GM.gmsd(vs, vh)) - want) <= 1e-6
    assert calls == []
    assert abs(float(GM.gmsd_loss(s, h)) - want) <= 1e-6
    assert calls == [1]


def test_refusals_on_the_gpu(A, monkeypatch):
    launched = []
    monkeypatch.setattr(A._lib, "call", lambda *a, **k: launched.append(a[0]))
    x2 = torch.rand(1, 2, 16, 16, device="cuda")
    for fn in (A.ops.gmsd_loss, A.ops.GMSDLossFn.apply, A.ops.gmsd):
        with pytest.raises(ValueError):
            fn(x2, x2)
        with pytest.raises(ValueError):
            fn(torch.rand(1, 3, 16, 16, device="cuda"), torch.rand(1, 3, 16, 17, device="cuda"))
    assert launched == [], "refused before any launch"


def _fit(A, precision, use_graph, losses="0.9*l1+0.1*gmsd"):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision=precision, n_feats=32, n_resblocks=2, res_scale=0.1, losses=losses)
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 400 + i, "cpu") for i in range(8)))
    torch.cuda.synchronize()
    return tr, [p.detach().clone() for p in m.parameters()]


def test_graphed_step_with_gmsd_follows_the_eager_loop(A):
    (tg, pg), (te, pe) = _fit(A, 32, True), _fit(A, 32, False)
    g = tg.graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step with the GMSD loss was captured"
    lg, le = tg.losses, te.losses
    assert len(lg) == len(le) == 8 and all(np.isfinite(lg))
    # every launch of the step sums in a fixed order ("Reproducibility"): the replayed step gives the eager loop's bits
    assert np.array_equal(np.asarray(lg, np.float32).view(np.int32), np.asarray(le, np.float32).view(np.int32)), (lg, le)
    for a, b in zip(pg, pe):
        assert torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), float((a - b).abs().max())
