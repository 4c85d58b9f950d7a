"""Large-kernel convolutions and the collapsed HR stage's forward kernel, element by element on rounded inputs."""


import os


import sys


import numpy as np


import pytest


import torch


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


sys.path.insert(0, ROOT)


from oracle import train as OT  # noqa: E402


sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


import dispatch_cases as D  # noqa: E402


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.rand(*s, generator=g) - 0.5).cuda()) for s in [(3,), (64, 64, 3, 3), (4097,), (7, 5, 3, 3)]]


def _grads(ps, step, scale):
    g = torch.Generator().manual_seed(77 + step)
    for i, p in enumerate(ps):
        p.grad = ((torch.rand(*p.shape, generator=g) - 0.5) * (10.0 ** (i % 3 - 1)) * scale).to(p.device)


# ---------------------------------------------------------------------------------------------------------------
# the direct large-kernel kernels per ELEMENT against float64 computed from the 16-bit-ROUNDED
# inputs (what is left is accumulation order, <= 1e-3 relative): a packing-permutation slip that touched one (kw, co) pair in 32
# passes a relative-L2 bound of 8 %, not this one
# ---------------------------------------------------------------------------------------------------------------
# the kernel families (forward, data gradient, weight gradient: srk_last_kernel()) each `path` of the test below stands for
PATH_KERNELS = {
    "lk_wgrad_allrows / lk_conv_rows": ("lk_conv_rows<9>", "lk_conv<2,2,9>", "lk_wgrad_allrows<9>"),
    "allrows": ("lk_conv_rows<9>", "lk_conv<2,2,9>", "lk_wgrad_allrows<9>"),
    "lk_wgrad_packed": ("lk_conv<8,1,5>", "lk5_dgrad", "lk_wgrad_packed<5>"),
    "allrows, 7x7": ("lk_conv_rows<7>", "lk_conv<2,2,7>", "lk_wgrad_allrows<7>"),
    "lk_wgrad": ("lk_conv<8,1,7>", "lk_conv<2,2,7>", "lk_wgrad<7>"),
    "lk5_wgrad": ("lk_conv<8,1,5>", "lk5_dgrad", "lk5_wgrad"),
    "lk5_wgrad (the collapsed HR stage's shape)": ("lk_conv<8,1,5>", "lk5_dgrad", "lk5_wgrad"),
    # 2 x 2 ragged 16-pixel tiles = 3 x 2 ragged 8-row tiles: a partial tile in both directions and more than one tile per direction
    "allrows, 5x5": ("lk_conv_rows<5>", "lk5_dgrad", "lk_wgrad_allrows<5>"),
    "lk_wgrad, 9x9": ("lk_conv<8,1,9>", "lk_conv<2,2,9>", "lk_wgrad<9>"),
}


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k,cout,n,h,w,path", [(9, 3, 2, 40, 33, "lk_wgrad_allrows / lk_conv_rows"), (9, 1, 1, 35, 20, "allrows"), (5, 6, 1, 33, 33, "lk_wgrad_packed"),
                                                (7, 4, 2, 16, 47, "allrows, 7x7"), (7, 16, 2, 17, 30, "lk_wgrad"), (5, 8, 1, 21, 19, "lk5_wgrad"),
                                                (5, 12, 3, 48, 48, "lk5_wgrad (the collapsed HR stage's shape)"), (5, 3, 1, 17, 18, "allrows, 5x5"),
                                                (9, 16, 1, 17, 18, "lk_wgrad, 9x9")])
def test_large_kernel_convs_per_element_on_rounded_inputs(A, dt, k, cout, n, h, w, path):
    import torch.nn.functional as F
    from sr_amd import ops
    g = torch.Generator().manual_seed(17 + k + cout)
    x = (torch.rand(n, 64, h, w, generator=g) * 2 - 1).to(dt)
    wt = (((torch.rand(cout, 64, k, k, generator=g) * 2 - 1) / np.sqrt(64 * k * k)).to(dt)).float()      # weights already representable
    b = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    gy = (torch.rand(n, cout, h, w, generator=g) * 2 - 1).to(dt)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    with D.Recorder() as rec:
        y = ops.conv_general(xd, wd, bd, stride=1, pad=k // 2)
        cp = y.shape[3]
        gyd = torch.zeros(n, h, w, cp, dtype=dt)
        gyd[..., :cout] = gy.permute(0, 2, 3, 1)
        y.backward(gyd.cuda())
        torch.cuda.synchronize()
    # the premise: the kernels `path` names are the ones that ran (forward, data gradient; weight gradient)
    assert (*D._names(rec.log, "srk_conv2d"), *D._names(rec.log, "srk_conv2d_wgrad")) == PATH_KERNELS[path], (path, rec.log)
    x64, w64, b64 = x.double().requires_grad_(True), wt.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv2d(x64, w64, b64, padding=k // 2)
    ref.backward(gy.double())
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    yy = y.detach().float().cpu()[..., :cout].permute(0, 3, 1, 2).double()
    r = ref.detach()
    # forward: one rounding of the stored output per element
    assert float((yy - r).abs().max()) <= 1.1 * eps * float(r.abs().max()) + 1e-6, path
    assert float(y.detach().float()[..., cout:].abs().max()) == 0.0 if cp > cout else True
    gx = xd.grad.float().cpu().permute(0, 3, 1, 2).double()
    assert float((gx - x64.grad).abs().max()) <= 1.1 * eps * float(x64.grad.abs().max()) + 1e-6, path
    # weight / bias gradients: fp32 sums of exact products of 16-bit values
    assert float((wd.grad.cpu().double() - w64.grad).abs().max()) <= 1e-3 * float(w64.grad.abs().max()), path
    assert float((bd.grad.cpu().double() - b64.grad).abs().max()) <= 1e-3 * float(b64.grad.abs().max()) + 1e-5, path


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("O,n,h,w", [(3, 2, 96, 96), (3, 3, 37, 61), (3, 1, 5, 29), (2, 2, 16, 28), (1, 1, 9, 57), (3, 17, 48, 48), (4, 2, 20, 33)])
def test_collapsed_stage_forward_kernel_per_element(A, dt, O, n, h, w):
    """lk5_rows_fwd_kernel ((kernel column, channel) pairs on the MFMA rows, weights in registers, column taps summed through a per-wave
    scratch; O = 4: the tap-per-MFMA kernel) against float64 conv2d + pixel_shuffle on the SAME 16-bit inputs: the image is stored in
    fp32, so what is left is the order of fp32 sums -- a slip in the row / column bookkeeping (band edges, row segments, the ring) is O(1)."""
    got, ins = D.collapsed_fwd_one(dt, O, n, h, w)          # (the launch and the reference are shared with test_gpu_dispatch_sides.py)
    ref = D.collapsed_ref(*ins)
    assert bool(torch.isfinite(got).all()), "pixels the kernel never wrote"
    assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_collapsed_stage_forward_walks_more_tiles_than_workgroups(A, dt):
    """lk5_fwd_kernel (4-colour images, no knob) is persistent: min(ntiles, CUs) workgroups, each walks ntiles // slots tiles and the first
    ntiles % slots of them one more (lk5_fwd_launch, csrc/conv_lk.hip).  CUs // 4 + 9 images of 17 x 20 are four ragged tiles each: every
    workgroup has a full round and the first 36 or so a second one.  Criterion of test_collapsed_stage_forward_kernel_per_element, for
    every image on its own, so that a failure names the images of the partial round."""
    O, h, w = 4, 17, 20
    cus = A._lib.load().srk_device_cus()
    n = cus // 4 + 9
    ntiles = n * ((h + 15) // 16) * ((w + 15) // 16)
    slots = min(ntiles, cus)                                      # the launcher's formula, restated: the premise of this test
    assert ntiles == 4 * n and ntiles // slots >= 1 and ntiles % slots != 0, (cus, n, ntiles, slots)
    with D.Recorder() as rec:
        got, ins = D.collapsed_fwd_one(dt, O, n, h, w)
    assert D._names(rec.log, "srk_conv2d") == ["lk5_fwd"], rec.log
    ref = D.collapsed_ref(*ins)
    assert bool(torch.isfinite(got).all()), ("pixels the kernel never wrote, images", torch.nonzero(~torch.isfinite(got).flatten(1).all(1)).flatten().tolist())
    err = (got - ref).abs().flatten(1).max(1).values
    bad = torch.nonzero(err > 2e-5 * float(ref.abs().max())).flatten().tolist()
    assert not bad, (f"images {bad} of {n} ({ntiles} tiles, {slots} workgroups, the first {ntiles % slots} walk one tile more)", float(err.max()))
