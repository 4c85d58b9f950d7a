"""HaarPSI on the MI355X (csrc/haarpsi.hip through sr_amd.haarpsi): the HIP loss and gradient against the float64 statement
of tests/haarpsi_ref.py, determinism, the upstream gradient, the index, the torch fallbacks and the graphed training step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import haarpsi_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _images(shape, seed, spill=True):
    """HR-like smooth images with fine texture and a saturated corner; SR = HR + noise, partly outside [0, 1] when `spill`."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    hr = torch.nn.functional.interpolate(torch.rand(n, c, max(2, h // 8), max(2, w // 8), generator=g), size=(h, w), mode="bilinear",
                                         align_corners=False)
    hr = (hr + 0.15 * torch.rand(n, c, h, w, generator=g)).clamp(0, 1)
    hr[:, :, : h // 4, : w // 4] = 1.0
    sr = hr + 0.05 * torch.randn(n, c, h, w, generator=g)
    if spill:
        sr[:, :, h // 2:, : w // 3] += 0.3                 # a region pushed above 1
        sr[:, :, : h // 3, w // 2:] -= 0.3                 # and one below 0
    return sr, hr


def _hip_loss_grad(A, sr, hr, weight=1.0):
    s = sr.detach().cuda().float().contiguous().requires_grad_(True)
    loss = A.ops.HaarPSILossFn.apply(s, hr.cuda().float().contiguous())
    (weight * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), s.grad.detach()


def _ref_loss_grad(sr, hr):
    s = sr.detach().double().requires_grad_(True)
    loss = REF.haarpsi_loss(s, hr.double())
    loss.backward()
    return loss.detach(), s.grad


# Calibration (the plain fp32 torch statement against float64 on such inputs): |d loss| <= 1.6e-6, relative L2 <= 4e-4, max
# <= 2.3e-3 of the largest entry (a max / abs branch flipped by fp32 rounding).
SHAPES = [(1, 3, 16, 16), (2, 3, 37, 50), (2, 3, 50, 37), (3, 3, 33, 33), (2, 1, 64, 48), (16, 3, 192, 192), (1, 3, 678, 1020)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_hip_matches_float64(A, shape):
    sr, hr = _images(shape, 11 + sum(shape))
    loss, g = _hip_loss_grad(A, sr, hr)
    l64, g64 = _ref_loss_grad(sr, hr)
    g = g.cpu().double()
    dl = abs(float(loss) - float(l64))
    l2 = float((g - g64).norm() / g64.norm())
    worst = float((g - g64).abs().max()) / float(g64.abs().max())
    print(f"\n{shape}: loss {float(loss):.6f}, |dloss| {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert torch.isfinite(g).all()
    assert dl <= 1e-5
    assert l2 <= 1e-3
    assert worst <= 1e-2
    outside = (sr < 0) | (sr > 1)
    assert outside.any() and float(g[outside].abs().max()) == 0.0


def test_deterministic(A):
    sr, hr = _images((4, 3, 96, 80), 3)
    l1, g1 = _hip_loss_grad(A, sr, hr)
    l2, g2 = _hip_loss_grad(A, sr, hr)
    assert float(l1) == float(l2) and torch.equal(g1, g2), "fixed-order reductions: bit-identical runs"


def test_upstream_gradient(A):
    sr, hr = _images((2, 3, 64, 72), 4)
    l1, g1 = _hip_loss_grad(A, sr, hr)
    l3, g3 = _hip_loss_grad(A, sr, hr, weight=3.5)
    assert float(l3) == float(l1)
    assert torch.allclose(g3, 3.5 * g1, rtol=1e-6, atol=0.0)


def test_index_is_one_minus_loss(A):
    sr, hr = _images((3, 3, 48, 40), 5)
    s, h = sr.cuda(), hr.cuda()
    loss = A.ops.haarpsi_loss(s, h)
    idx = A.ops.haarpsi(s, h)
    assert idx.dim() == 0 and idx.is_cuda
    assert abs(float(idx) - (1.0 - float(loss))) <= 1.2e-7
    assert abs(float(idx) - float(REF.haarpsi_index(sr.clamp(0, 1).double(), hr.double()))) <= 1e-5


def test_fallbacks_take_the_torch_path(A, monkeypatch):
    calls = []
    real = A.ops.HaarPSILossFn.apply
    monkeypatch.setattr(A.ops.HaarPSILossFn, "apply", lambda *a: calls.append(1) or real(*a))
    from sr_amd import haarpsi as HP
    sr, hr = _images((2, 3, 32, 32), 6)
    s, h = sr.cuda(), hr.cuda()
    want = float(REF.haarpsi_loss(sr.double(), hr.double()))
    # hr needing a gradient, float64 inputs and C = 2 go to haarpsi_torch
    hg = h.clone().requires_grad_(True)
    assert abs(float(HP.haarpsi_loss(s, hg).detach()) - want) <= 1e-5
    assert abs(float(HP.haarpsi_loss(s.double(), h.double())) - want) <= 1e-10
    s2, h2 = s[:, :2].contiguous(), h[:, :2].contiguous()
    assert abs(float(HP.haarpsi_loss(s2, h2)) - float(REF.haarpsi_loss(s2.cpu().double(), h2.cpu().double()))) <= 1e-5
    assert calls == []
    HP.haarpsi_loss(s, h)
    assert calls == [1]


def _fit(A, precision, use_graph, losses="0.9*l1+0.1*haarpsi"):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision=precision, n_feats=32, n_resblocks=2, res_scale=0.1, losses=losses)
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 400 + i, "cpu") for i in range(8)))
    torch.cuda.synchronize()
    return tr, [p.detach().clone() for p in m.parameters()]


def test_graphed_step_with_haarpsi_follows_the_eager_loop(A):
    (tg, pg), (te, pe) = _fit(A, 32, True), _fit(A, 32, False)
    g = tg.graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step with the HaarPSI loss was captured"
    lg, le = tg.losses, te.losses
    assert len(lg) == len(le) == 8 and all(np.isfinite(lg))
    # every launch of the step sums in a fixed order ("Reproducibility"): the replayed step gives the eager loop's bits
    assert np.array_equal(np.asarray(lg, np.float32).view(np.int32), np.asarray(le, np.float32).view(np.int32)), (lg, le)
    for a, b in zip(pg, pe):
        assert torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), float((a - b).abs().max())


def test_graphed_fp16_step_with_haarpsi(A):
    (tg, pg), (te, pe) = _fit(A, 16, True), _fit(A, 16, False)
    assert tg.scaler is not None and hasattr(tg.scaler, "state")
    g = tg.graphed
    assert g is not None and g.graphs is not None and not g.failed
    lg, le = tg.losses, te.losses
    assert len(lg) == 8 and all(np.isfinite(lg))
    # the loss scaler's launches are part of the captured step and every sum has a fixed order: fp16 replays the eager loop's bits too
    assert np.array_equal(np.asarray(lg, np.float32).view(np.int32), np.asarray(le, np.float32).view(np.int32)), (lg, le)
    for a, b in zip(pg, pe):
        assert torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), float((a - b).abs().max())
