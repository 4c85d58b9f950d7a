"""FLIP on the MI355X (csrc/flip.hip through sr_amd.flip): the HIP forward / backward against the reference's fixtures and
against flip_torch in float64, determinism, the upstream gradient, composite losses, the graphed training step and the
validation metric."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "flip_*.npz")))

# the criteria of tests/test_flip_cpu.py (fp32 vs the reference's fp32 result)
LOSS_RTOL, MAP_ATOL, GRAD_ATOL_REL = 1e-5, 2e-4, 2e-2


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _hip_loss_grad(A, sr, hr, weight=1.0):
    s = sr.detach().cuda().float().contiguous().requires_grad_(True)
    loss = A.ops.FlipLossFn.apply(s, hr.cuda().float().contiguous())
    (weight * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), s.grad.detach()


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[5:-4] for p in FIXTURES])
def test_hip_matches_the_reference_fixtures(A, path):
    z = dict(np.load(path))
    sr, hr = torch.tensor(z["sr"]), torch.tensor(z["hr"])
    loss, g = _hip_loss_grad(A, sr, hr)
    ref = float(z["loss"])
    assert abs(float(loss) - ref) <= LOSS_RTOL * ref, (float(loss), ref)
    emap = A.ops.flip_error_map(sr.cuda(), hr.cuda()).cpu().numpy()[:, 0]
    assert float(np.abs(emap - z["err"]).max()) <= MAP_ATOL
    assert abs(float(A.ops.flip(sr.cuda(), hr.cuda())) - float(loss)) == 0.0
    g = g.cpu().numpy()
    rg = z["grad"]
    assert np.isfinite(g).all()
    fin = np.isfinite(rg)
    d = float(np.abs(g[fin] - rg[fin]).max())
    assert d <= GRAD_ATOL_REL * float(np.abs(rg[fin]).max()), d


def _images(n, h, w, seed):
    """HR-like smooth images with a few saturated patches, and an SR-like estimate (blurred + noise, partly out of [0,1])."""
    g = torch.Generator().manual_seed(seed)
    hr = torch.nn.functional.interpolate(torch.rand(n, 3, max(1, h // 8), max(1, w // 8), generator=g), size=(h, w), mode="bilinear",
                                         align_corners=False)
    hr = (hr + 0.1 * torch.rand(n, 3, h, w, generator=g)).clamp(0, 1)
    if h >= 16 and w >= 16:
        hr[:, :, : h // 4, : w // 4] = 1.0
    sr = hr + 0.04 * torch.randn(n, 3, h, w, generator=g)
    return sr, hr


# HIP (fp32) against flip_torch in float64 on the GPU.  Measured spread of flip_torch in fp32 against float64 (same inputs):
#   16x3x192x192  loss 3e-8 rel, map 5e-6; gradient: relative L2 2.7e-4, 3.4e-6 of the entries off by more than 1 % of the
#                 largest entry, the worst 1.6 % of it (a few pixels next to a singular point: the feature term's slope grows as
#                 1 / sqrt(Fe) when Fe -> 0, and the max / clamp kinks decide on rounded values)
#   1x3x339x510   relative L2 3.8e-4, 5.8e-6 of the entries beyond 1 %, the worst 2.4 %
# The bounds: 5x the measured relative L2 and fraction, a worst entry under 10 %; loss and map as in test_flip_cpu.py.
@pytest.mark.parametrize("shape", [(16, 192, 192), (256, 192, 192), (1, 339, 510), (1, 7, 5), (2, 1, 64)],
                         ids=["16x192", "256x192", "339x510", "7x5", "1x64"])
def test_hip_matches_float64(A, shape):
    n, h, w = shape
    sr, hr = _images(n, h, w, 7 + h + w)
    loss, g = _hip_loss_grad(A, sr, hr)
    s64 = sr.cuda().double().requires_grad_(True)
    e64 = A.ops.flip_error_map_torch(s64, hr.cuda().double())
    l64 = e64.mean()
    l64.backward()
    rel = abs(float(loss) - float(l64.detach())) / float(l64.detach())
    emap = A.ops.flip_error_map(sr.cuda(), hr.cuda())
    dmap = float((emap.double() - e64.detach()).abs().max())
    g64 = s64.grad
    d = (g.double() - g64).abs()
    m = float(g64.abs().max())
    worst, l2 = float(d.max()) / m, float((g.double() - g64).norm() / g64.norm())
    frac = float((d > 1e-2 * m).double().mean())
    print(f"\n{shape}: loss rel {rel:.2e}, map max abs {dmap:.2e}, grad rel L2 {l2:.2e}, beyond 1 % {frac:.2e}, worst {worst:.2e}")
    assert torch.isfinite(g).all()
    assert rel <= LOSS_RTOL
    assert dmap <= MAP_ATOL
    assert l2 <= 2e-3 and frac <= 3e-5 and worst <= 0.1


def test_deterministic_and_upstream_gradient(A):
    sr, hr = _images(4, 96, 80, 3)
    l1, g1 = _hip_loss_grad(A, sr, hr)
    l2, g2 = _hip_loss_grad(A, sr, hr)
    assert float(l1) == float(l2) and torch.equal(g1, g2), "fixed-order reduction: bit-identical runs"
    l3, g3 = _hip_loss_grad(A, sr, hr, weight=3.0)
    assert float(l3) == float(l1)
    assert torch.allclose(g3, 3.0 * g1, rtol=1e-6, atol=0.0)


def test_composite_loss_hip_vs_torch(A):
    """0.7 * l1 + 0.3 * flip: the HIP path and the torch path (hr requiring a gradient routes flip_loss to flip_torch)."""
    sr, hr = _images(3, 64, 64, 5)
    out = []
    for torch_path in (False, True):
        s = sr.cuda().requires_grad_(True)
        h = hr.cuda().requires_grad_(torch_path)
        loss = 0.7 * torch.nn.functional.l1_loss(s, h) + 0.3 * A.ops.flip_loss(s, h)
        loss.backward()
        out.append((float(loss), s.grad.clone()))
    (la, ga), (lb, gb) = out
    assert abs(la - lb) <= 1e-5 * abs(lb)
    assert float((ga - gb).abs().max()) <= 2e-2 * float(gb.abs().max())


def _fit(A, precision, use_graph, losses="l1+flip"):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision=precision, n_feats=32, n_resblocks=2, res_scale=0.1, losses=losses)
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 400 + i, "cpu") for i in range(8)))
    torch.cuda.synchronize()
    return tr, [p.detach().clone() for p in m.parameters()]


def test_graphed_step_with_flip_follows_the_eager_loop(A):
    (tg, pg), (te, pe) = _fit(A, 32, True), _fit(A, 32, False)
    g = tg.graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step with the FLIP loss was captured"
    lg, le = tg.losses, te.losses
    assert len(lg) == len(le) == 8 and all(np.isfinite(lg))
    # every launch of the step sums in a fixed order ("Reproducibility"): the replayed step gives the eager loop's bits
    assert np.array_equal(np.asarray(lg, np.float32).view(np.int32), np.asarray(le, np.float32).view(np.int32)), (lg, le)
    for a, b in zip(pg, pe):
        assert torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), float((a - b).abs().max())


def test_graphed_fp16_step_with_flip(A):
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


def test_validation_metric_flip(A):
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision=32, n_feats=32, n_resblocks=2, res_scale=0.1, metrics=["PSNR", "SSIM", "FLIP"],
               eval_datasets=["X"]).cuda()
    g = torch.Generator().manual_seed(2)
    lr, hr = torch.rand(1, 3, 40, 52, generator=g).cuda(), torch.rand(1, 3, 80, 104, generator=g).cuda()
    res = m.validation_step({"lr": lr, "hr": hr}, 0)
    with torch.no_grad():
        sr = m(lr).clamp(0, 1)
    want = float(A.ops.flip_torch(sr.double(), hr.double()))
    assert abs(float(res["X/FLIP"]) - want) <= 1e-5 * want
    assert {"X/PSNR", "X/SSIM", "X/FLIP"} <= set(res)
