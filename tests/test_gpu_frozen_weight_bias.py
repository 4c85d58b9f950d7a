"""A conv with a frozen weight and a trainable bias: the bias gets its gradient (each parameter is gated on its own
`needs_input_grad`), the weight gets none -- through `conv`, `conv_chain` (pair launch and per-layer launches) and `res_trunk`,
against float64 torch.  Weights and upstream gradient are positive, so that the bias gradients (sums over all pixels) do not cancel
and the bf16 rounding of the intermediates stays far below the tolerance."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


def _convs(n, seed):
    g = torch.Generator().manual_seed(seed)
    ws = [torch.nn.Parameter((torch.rand(64, 64, 3, 3, generator=g) * 0.02).cuda(), requires_grad=False) for _ in range(n)]
    bs = [torch.nn.Parameter(((torch.rand(64, generator=g) - 0.5) * 0.1).cuda()) for _ in range(n)]
    return ws, bs


def _inputs(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand(n, hw, hw, 64, generator=g) - 0.5) * 2).to(torch.bfloat16).cuda().requires_grad_(True)
    t = torch.rand(n, hw, hw, 64, generator=g).to(torch.bfloat16).float().cuda()      # upstream gradient, exact in bf16
    return x, t


def _check(ws, bs, ref_fn, x, t):
    """Bias gradients against float64 torch of the same network; frozen weights get no .grad."""
    xd = x.detach().double().cpu().permute(0, 3, 1, 2)
    wd = [w.detach().double().cpu() for w in ws]
    bd = [b.detach().double().cpu().requires_grad_(True) for b in bs]
    (ref_fn(xd, wd, bd) * t.double().cpu().permute(0, 3, 1, 2)).sum().backward()
    for i, (w, b, r) in enumerate(zip(ws, bs, bd)):
        assert w.grad is None, f"frozen weight {i} got a gradient"
        assert b.grad is not None, f"bias {i} got no gradient"
        err = float((b.grad.double().cpu() - r.grad).norm() / r.grad.norm())
        assert err < 2e-2, (i, err)


def _chain_ref(relus, scale):
    def f(x, ws, bs):
        a = x
        for i, (w, b) in enumerate(zip(ws, bs)):
            a = F.conv2d(a, w, b, padding=1)
            if relus[i]:
                a = torch.relu(a)
        return a * scale + x
    return f


def test_frozen_weight_trainable_bias_conv(A):
    ws, bs = _convs(1, 1)
    x, t = _inputs(2, 24, 2)
    (A.ops.conv(x, ws[0], bs[0], scale=0.5).float() * t).sum().backward()
    torch.cuda.synchronize()
    _check(ws, bs, lambda x_, w_, b_: F.conv2d(x_, w_[0], b_[0], padding=1) * 0.5, x, t)


@pytest.mark.parametrize("paired", [True, False])
def test_frozen_weight_trainable_bias_conv_chain(A, paired):
    relus = [True, False] if paired else [True, True, False]
    ws, bs = _convs(len(relus), 3)
    x, t = _inputs(2, 24, 4)
    assert A.ops.pair_ok(x, ws[0], ws[1]), "a small batch: the two-conv chain runs as the pair launch"
    before = A.ops.PAIR_LAUNCHES[0]
    y = A.ops.conv_chain(x, list(zip(ws, bs)), relus, scale=0.5)
    assert (A.ops.PAIR_LAUNCHES[0] > before) == paired
    (y.float() * t).sum().backward()
    torch.cuda.synchronize()
    _check(ws, bs, _chain_ref(relus, 0.5), x, t)


def test_frozen_weight_trainable_bias_res_trunk(A):
    nb, scale = 2, 0.5
    ws, bs = _convs(2 * nb + 1, 5)
    x, t = _inputs(A._lib.load().srk_device_cus(), 8, 6)
    blocks = [((ws[2 * i], bs[2 * i]), (ws[2 * i + 1], bs[2 * i + 1])) for i in range(nb)]
    tail = (ws[2 * nb], bs[2 * nb])
    assert A.ops.res_trunk_ok(x, blocks, tail)
    (A.ops.res_trunk(x, blocks, tail, scale).float() * t).sum().backward()
    torch.cuda.synchronize()

    def ref(x_, w_, b_):
        a = x_
        for i in range(nb):
            h = torch.relu(F.conv2d(a, w_[2 * i], b_[2 * i], padding=1))
            a = a + scale * F.conv2d(h, w_[2 * i + 1], b_[2 * i + 1], padding=1)
        return F.conv2d(a, w_[2 * nb], b_[2 * nb], padding=1) + x_
    _check(ws, bs, ref, x, t)
