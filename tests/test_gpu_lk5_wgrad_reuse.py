"""The 5x5 weight gradient of the collapsed HR stage (csrc/conv_lk.hip: lk5_wgrad_kernel, 64 input x 16 stored gradient channels of
which 12 are real) against the float64 correlation of the same 16-bit-rounded inputs, TAP BY TAP.

The kernel deals its 14 tap pairs to two wave halves and feeds pair t + 5 from a two-row register delay line of pair t's fragments
instead of a second LDS read.  A wrong pair-to-wave map, a swapped t / t + 5 or a line that lags by one row puts a whole tap's sum
under another tap (or another row's gradient under the right tap), so every tap is compared on its own.  Shapes: one tile (the line is
filled and used inside it); ragged tiles in both directions, several per workgroup (the line restarts at every tile); fewer rows than a
tile (rows beyond the image reach the line as zeros); single pixels on two opposite edges (every halo row empty).

Entry, comparison and tolerances are those of tests/test_gpu_conv_lk_float64.py (relative L2 error, 8e-2 bf16 / 3e-2 fp16); a tap whose
float64 sum is exactly zero (no pixel pair that far apart in so small an image) must come out exactly zero."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L2 = {torch.bfloat16: 8e-2, torch.float16: 3e-2}          # tests/test_gpu_conv_lk_float64.py: l2 of the weight / bias gradients
SHAPES = [(1, 16, 16), (2, 17, 33), (3, 5, 40), (1, 1, 1), (1, 2, 1)]
K, CIN, COUT = 5, 64, 12


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


def _inputs(n, h, w, one_pixel):
    g = torch.Generator().manual_seed(11 + 100 * h + w)
    x = torch.rand(n, CIN, h, w, generator=g) * 2 - 1
    gy = torch.rand(n, COUT, h, w, generator=g) * 2 - 1
    if one_pixel:           # the gradient lives in ONE pixel (off-centre where the image allows): tap f sees exactly x[pixel + f]
        keep = torch.zeros(n, 1, h, w)
        keep[n - 1, 0, (2 * h) // 3, w // 3] = 1.0
        gy = gy * keep
    return x, gy


def _float64(x, gy, dt):
    """dW [12, 64, 5, 5] and db [12] of a 5x5 'same' convolution, from the 16-bit-rounded x and gy, in float64."""
    import torch.nn.functional as F
    xr, gr = x.to(dt).double(), gy.to(dt).double()
    w0 = torch.zeros(COUT, CIN, K, K, dtype=torch.float64, requires_grad=True)
    b0 = torch.zeros(COUT, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w0, b0, padding=K // 2).backward(gr)
    return w0.grad, b0.grad


_REF = {}


def _ref(shape, one_pixel, dt):
    key = (shape, one_pixel, dt)
    if key not in _REF:
        x, gy = _inputs(*shape, one_pixel)
        _REF[key] = (x, gy) + _float64(x, gy, dt)
    return _REF[key]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("one_pixel", [False, True], ids=["dense", "one_pixel"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lk5_wgrad_every_tap_vs_float64(A, shape, one_pixel, dt):
    from sr_amd import ops
    n, h, w = shape
    x, gy, dw_ref, db_ref = _ref(shape, one_pixel, dt)
    g = torch.Generator().manual_seed(3)
    wt = (torch.rand(COUT, CIN, K, K, generator=g) * 2 - 1) / np.sqrt(CIN * K * K)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dt).cuda().requires_grad_(True)
    wd, bd = torch.nn.Parameter(wt.cuda()), torch.nn.Parameter(torch.zeros(COUT).cuda())
    y = ops.conv_general(xd, wd, bd, stride=1, pad=K // 2)
    assert y.shape[3] == 16, "the 12 gradient channels are stored as 16: the geometry of the collapsed HR stage"
    gyd = torch.zeros(n, h, w, 16, dtype=dt)
    gyd[..., :COUT] = gy.permute(0, 2, 3, 1).to(dt)
    y.backward(gyd.cuda())
    torch.cuda.synchronize()
    dw, db = wd.grad.double().cpu(), bd.grad.double().cpu()
    assert dw.shape == dw_ref.shape and db.shape == db_ref.shape

    def l2e(a_, b_):
        return float((a_ - b_).norm() / b_.norm())

    bad = []
    for fy in range(K):
        for fx in range(K):
            got, want = dw[:, :, fy, fx], dw_ref[:, :, fy, fx]
            if float(want.abs().max()) == 0.0:
                e = 0.0 if float(got.abs().max()) == 0.0 else float("inf")
            else:
                e = l2e(got, want)
            if not e < L2[dt]:
                bad.append(((fy - 2, fx - 2), e))
    assert not bad, f"taps (fy, fx) with their relative L2 error: {bad}"
    assert l2e(dw, dw_ref) < L2[dt]
    assert l2e(db, db_ref) < L2[dt]
