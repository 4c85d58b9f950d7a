"""MS-SSIM on the MI355X (csrc/ms_ssim.hip through ops.ms_ssim): the result and every level's cs / ss against the float64 statement
in tests/ms_ssim_ref.py, closed forms, determinism, no host sync, the model's validation path and the C ABI's refusals."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ms_ssim_ref as R  # noqa: E402
from test_ms_ssim_cpu import SHAPES, images  # noqa: E402

GPU_SHAPES = SHAPES + [(1, 3, 1356, 2040), (4, 3, 192, 192)]


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=["x".join(map(str, s)) for s in GPU_SHAPES])
def test_matches_float64_per_level(A, shape):
    sr, hr = images(shape, seed=sum(shape))
    ref = R.ms_ssim(sr, hr)
    got, cs, ss = A.ops.ms_ssim_levels(sr.cuda(), hr.cuda())
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
    assert abs(float(got) - float(ref["value"])) <= 2e-5, (float(got), float(ref["value"]))
    assert float((cs.cpu() - ref["cs"]).abs().max()) <= 2e-5
    assert float((ss.cpu() - ref["ss"]).abs().max()) <= 2e-5
    assert float(A.ops.ms_ssim(sr.cuda(), hr.cuda())) == float(got)


def test_identical_constant_and_negated(A):
    sr, _ = images((2, 3, 200, 180), seed=5)
    x = sr.cuda()
    assert abs(float(A.ops.ms_ssim(x, x)) - 1.0) <= 1e-6
    a, b = 0.25, 0.75
    want = ((2 * a * b + 1e-4) / (a * a + b * b + 1e-4)) ** 0.1333
    got = float(A.ops.ms_ssim(torch.full((1, 3, 170, 190), a, device="cuda"), torch.full((1, 3, 170, 190), b, device="cuda")))
    assert abs(got - want) <= 1e-5, (got, want)
    assert float(A.ops.ms_ssim(x, 1.0 - x)) == 0.0


def test_bf16_input(A):
    sr, hr = images((1, 3, 192, 200), seed=11)
    s16, h16 = sr.cuda().bfloat16(), hr.cuda().bfloat16()
    got = float(A.ops.ms_ssim(s16, h16))
    want = float(R.ms_ssim(s16.float().cpu(), h16.float().cpu())["value"])
    assert abs(got - want) <= 2e-5


def test_bit_reproducible(A):
    sr, hr = images((2, 3, 321, 481), seed=3)
    x, y = sr.cuda(), hr.cuda()
    r = [A.ops.ms_ssim_levels(x, y) for _ in range(2)]
    assert torch.equal(r[0][0], r[1][0]) and torch.equal(r[0][1], r[1][1]) and torch.equal(r[0][2], r[1][2])


def test_no_host_sync(A):
    """(1) With the stream held busy by a long device-side sleep, the call returns while the sleep is still running: it never
    waited for the device.  (2) Where torch's sync debug mode is effective on this build (a synchronising .item() raises under
    it), the call runs under it without raising."""
    sr, hr = images((1, 3, 256, 256), seed=4)
    x, y = sr.cuda(), hr.cuda()
    out = A.ops.ms_ssim(x, y)                             # warm: library, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            x.sum().item()
            effective = False
        except RuntimeError:
            effective = True
        if effective:
            out = A.ops.ms_ssim(x, y)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    print(f"sync debug mode effective: {effective}")
    done = torch.cuda.Event()
    torch.cuda._sleep(200_000_000)
    out2 = A.ops.ms_ssim(x, y)
    done.record()
    assert not done.query()
    torch.cuda.synchronize()
    assert float(out) == float(out2)


def test_model_metric_and_validation_epoch(A):
    sr, hr = images((2, 3, 192, 176), seed=8)
    m = A.EDSR(scale_factor=2, precision=32, n_feats=32, n_resblocks=2, res_scale=0.1, metrics=["PSNR", "SSIM", "MS-SSIM"],
               eval_datasets=["X"]).cuda()
    res = m._calculate_metrics(img_sr=sr.cuda(), img_hr=hr.cuda())
    assert float(res["X/MS-SSIM"]) == float(A.ops.ms_ssim(sr.cuda(), hr.cuda()))
    g = torch.Generator().manual_seed(2)
    for i in range(2):
        lr = torch.rand(1, 3, 96, 88, generator=g).cuda()
        hr = torch.rand(1, 3, 192, 176, generator=g).cuda()
        out = m.validation_step({"lr": lr, "hr": hr}, i)
        with torch.no_grad():
            srm = m(lr).clamp(0, 1)
        assert abs(float(out["X/MS-SSIM"]) - float(R.ms_ssim(srm.cpu(), hr.cpu())["value"])) <= 2e-5
    means = m.on_validation_epoch_end()
    assert {"X/PSNR", "X/SSIM", "X/MS-SSIM"} <= set(means)
    assert torch.isfinite(torch.as_tensor(means["X/MS-SSIM"]))


def test_c_abi_refuses_and_mirrors_the_header(A):
    L = A._lib
    assert L.STRUCTS["srk_ms_ssim_args"] is L.MsSsimArgs       # its layout: tests/test_host_surface.py
    lib = L.load()
    x = torch.rand(1, 3, 200, 200, device="cuda")
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    out = torch.empty((), device="cuda")

    def args(**kw):
        d = dict(x=x.data_ptr(), y=x.data_ptr(), workspace=ws.data_ptr(), partials=ws.data_ptr() + (1 << 21), out=out.data_ptr(),
                 N=1, C=3, H=200, W=200, sigma=1.5, k1=0.01, k2=0.03, w0=0.0448, w1=0.2856, w2=0.3001, w3=0.2363, w4=0.1333)
        d.update(kw)
        return L.MsSsimArgs(**d)
    stream = torch.cuda.current_stream().cuda_stream
    for bad in (dict(H=160), dict(W=160), dict(x=0), dict(y=0), dict(workspace=0), dict(partials=0), dict(out=0), dict(N=70000)):
        assert lib.srk_ms_ssim(ctypes.byref(args(**bad)), ctypes.c_void_p(stream)) != 0, bad
    assert lib.srk_ms_ssim_workspace_bytes(1, 3, 160, 400) < 0 and lib.srk_ms_ssim_tiles(400, 160, None) < 0
    with pytest.raises(ValueError, match="expected at least 161x161"):
        A.ops.ms_ssim(x[..., :160, :], x[..., :160, :])
    with pytest.raises(ValueError):
        A.ops.ms_ssim(x, x[..., :199])
