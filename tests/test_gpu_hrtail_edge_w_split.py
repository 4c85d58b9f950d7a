"""srk_hrtail_edge_bwd_w + its chunk reduction (csrc/hr_tail.hip) at the batch sizes where the split of the work changes: one image
per chunk (N = 1, 3, 64), the switch of the images-per-chunk rule at 64 (N = 65: two images per chunk, the last chunk uneven) and
uneven chunks of three (N = 130).  An edge's items are sliced over gridDim.z workgroups; every (edge type, item) must come out
whichever workgroup owns it.

Oracle: the float64 statement of the border sums in tests/collapse_ref.py (np_border_sums) on the same 16-bit-rounded x and the same
fp32 g.  Tolerances: the parameter-gradient bounds of tests/test_gpu_hr_tail.py (relative L2 error 2e-2 bf16 / 3e-3 fp16), per edge
type and per corner so that a failure names the workgroup row that went wrong."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collapse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

O, C, CI = 3, 64, 64
TOL = {torch.bfloat16: 2e-2, torch.float16: 3e-3}


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


def _relerr(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hw", [(6, 7), (1, 4)], ids=["6x7", "1x4"])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 130])
def test_edge_weight_sums_vs_float64(A, n, hw, dt):
    L, ops = A._lib, A.ops
    h, w = hw
    dev, f32 = torch.device("cuda"), torch.float32
    gen = torch.Generator().manual_seed(17 * n + h)
    x = (torch.rand(n, h, w, CI, generator=gen) - 0.5).to(dt)
    g = torch.rand(n, O, 2 * h, 2 * w, generator=gen) - 0.5
    want = R.np_border_sums(x.double().permute(0, 3, 1, 2).numpy(), g.double().numpy())[2:]      # E, e0, K, k0

    wu = torch.zeros(4 * C, CI, 3, 3, device=dev)
    wt = torch.zeros(O, C, 3, 3, device=dev)
    xd, gd = x.to(dev), g.to(dev)
    red = dict(eedge=torch.full((4, 2 * O, CI, 5), float("nan"), dtype=f32, device=dev), e0=torch.full((4, 2 * O), float("nan"), dtype=f32, device=dev),
               ecor=torch.full((4, O, CI), float("nan"), dtype=f32, device=dev), k0=torch.full((4, O), float("nan"), dtype=f32, device=dev))
    scratch = torch.full((int(L.load().srk_hrtail_scratch_floats(n, CI)),), float("nan"), dtype=f32, device=dev)
    ptrs = {k: v.data_ptr() for k, v in red.items()}
    L.call("srk_hrtail_edge_bwd_w", ops.HrTailFn._args(xd, wu, None, wt, None, ops._hr_bufs(O, CI, dev), g=gd.data_ptr(), scratch=scratch.data_ptr(), **ptrs),
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = [red[k].double().cpu().numpy() for k in ("eedge", "e0", "ecor", "k0")]
    for name, a_, b_ in zip(("eedge", "e0", "ecor", "k0"), got, want):
        assert a_.shape == b_.shape, name
        assert np.isfinite(a_).all(), f"{name}: an item no workgroup wrote"
        for ty in range(4):             # the four edges / the four corners
            e = _relerr(a_[ty], b_[ty])
            assert e < TOL[dt], f"{name}[{ty}]: relative L2 error {e}"
