"""SSIM loss on the CPU: the float64 statement of tests/ssim_loss_ref.py grounded on the oracle's SSIM and on central differences,
`ssim_torch` in fp32 against it (the calibration the GPU limits rest on), the loss string, the clamp and pooling rules of the
gradient, the degenerate and refused inputs, the ctypes mirror of the header and train.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_loss_ref as REF  # noqa: E402
from oracle import metrics as OM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def SL():
    from sr_amd import ssim_loss
    return ssim_loss


# ---- the reference is grounded ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 27, 38), (1, 1, 384, 391)], ids=["f1", "f2"])
def test_reference_value_is_one_minus_the_oracle_ssim(shape):
    sr, hr = REF.images(shape, 21, spill=False)
    x = sr.clamp(0, 1).double()
    assert abs(float(REF.ssim_loss(x, hr)) - (1.0 - float(OM.ssim(x, hr.double())))) <= 1e-12


def test_reference_gradient_agrees_with_central_differences():
    """Central differences of the float64 loss, h = 1e-6, at corners, edges, interior pixels and pixels inside both clamped regions
    (there the loss does not move at all and the gradient is exactly 0).  1e-6 relative: of the pixel's own gradient where that is
    large enough to be resolved, and never worse than 1e-6 of the largest gradient entry.  (The difference quotient itself is only
    good to about eps * loss / h = 4e-11 absolute, which a corner pixel, whose single window weighs it 1e-6, does not rise above:
    the absolute floor is what such pixels are held to.)"""
    shape = (2, 3, 27, 38)
    sr, hr = REF.images(shape, 22)
    sr, hr = sr.double(), hr.double()
    _, g = REF.loss_and_grad(sr, hr)
    gmax = float(g.abs().max())
    h = 1e-6
    pixels = [(0, 0, 0, 0), (0, 0, 0, 37), (0, 1, 26, 0), (1, 2, 26, 37),                      # corners
              (0, 0, 0, 19), (0, 1, 13, 0), (1, 0, 26, 20), (1, 2, 12, 37),                    # edges
              (0, 0, 10, 14), (0, 1, 12, 16), (0, 2, 11, 15), (1, 0, 10, 15), (1, 1, 12, 17), (1, 2, 9, 16),   # interior, unclamped
              (0, 0, 3, 3), (1, 1, 5, 7)]                                                      # the saturated corner of hr
    above, below = torch.nonzero(sr > 1.0 + 1e-3), torch.nonzero(sr < -1e-3)                   # inside the clamped regions
    pixels += [tuple(int(i) for i in t[k]) for t in (above, below) for k in (len(t) // 3, 2 * len(t) // 3)]
    assert len(pixels) == 20
    clamped = 0
    for p in pixels:
        v = float(sr[p])
        assert min(abs(v), abs(v - 1.0)) > 10 * h, "not on the clamp's kink"
        up, dn = sr.clone(), sr.clone()
        up[p] += h
        dn[p] -= h
        fd = (float(REF.ssim_loss(up, hr)) - float(REF.ssim_loss(dn, hr))) / (2 * h)
        got = float(g[p])
        if v < 0.0 or v > 1.0:
            clamped += 1
            assert fd == 0.0 and got == 0.0, (p, fd, got)
        else:
            assert abs(fd - got) <= max(1e-6 * abs(got), 1e-7 * gmax), (p, fd, got, gmax)
            assert abs(fd - got) <= 1e-6 * gmax
    assert 4 <= clamped <= 8


# ---- ssim_torch in fp32 against the reference: the calibration ----------------------------------------------------------------
@pytest.fixture(scope="module")
def calibration(SL):
    out = {}
    for shape in REF.SHAPES:
        sr, hr = REF.images(shape, 11 + sum(shape))
        l64, g64 = REF.loss_and_grad(sr, hr)
        s = sr.clone().requires_grad_(True)
        loss = SL.ssim_loss(s, hr)
        loss.backward()
        out[shape] = REF.errors(loss.detach(), s.grad, l64, g64)
    return out


def test_fp32_torch_statement_leaves_the_gpu_limits_a_threefold_margin(calibration):
    """What fp32 arithmetic alone costs, on the GPU tests' own inputs and shapes.  Measured on the CPU over REF.SHAPES:
    |d loss| <= 6.3e-7, gradient relative L2 <= 2.8e-5, max error <= 3.8e-5 of the largest entry (without the half shift of
    ssim_loss.SHIFT: 2.8e-6, 1.2e-4, 1.7e-4).  Each is held to a third of the limit the HIP path is given (REF.LIMIT_*: 1e-5, 1e-3,
    3e-3), so those limits carry margin for the kernel's summation order over fp32 rounding itself."""
    for shape, (dl, l2, worst) in calibration.items():
        print(f"\n{shape}: |dloss| {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert max(v[0] for v in calibration.values()) <= REF.LIMIT_LOSS / 3
    assert max(v[1] for v in calibration.values()) <= REF.LIMIT_L2 / 3
    assert max(v[2] for v in calibration.values()) <= REF.LIMIT_MAX / 3


def test_float64_torch_statement_is_the_reference(SL):
    sr, hr = REF.images((2, 3, 27, 38), 23)
    l64, g64 = REF.loss_and_grad(sr, hr)
    s = sr.double().requires_grad_(True)
    loss = SL.ssim_loss(s, hr.double())
    loss.backward()
    assert abs(float(loss.detach()) - float(l64)) <= 1e-12
    assert float((s.grad - g64).abs().max()) <= 1e-10 * float(g64.abs().max())
    assert abs(float(SL.ssim_torch(sr.clamp(0, 1).double(), hr.double())) - float(REF.ssim_index(sr.clamp(0, 1), hr))) <= 1e-12


# ---- the loss string ------------------------------------------------------------------------------------------------------------
def test_model_accepts_the_l1_ssim_composite():
    import sr_amd
    m = sr_amd.SRCNN(scale_factor=2, losses="0.16*l1+0.84*ssim")
    assert [(l.name, l.weight) for l in m._losses] == [("l1", 0.16), ("ssim", 0.84)]
    sr, hr = REF.images((2, 3, 32, 32), 24)
    sr, hr = sr.float(), hr.float()
    out = m._calculate_losses(img_sr=sr, img_hr=hr)
    assert set(out) == {"loss", "loss/l1", "loss/ssim"}
    want = 0.16 * float(torch.nn.functional.l1_loss(sr.double(), hr.double())) + 0.84 * float(REF.ssim_loss(sr, hr))
    assert abs(float(out["loss"]) - want) <= 1e-5
    for losses in ("ssim", "l1 + 0.5*SSIM"):
        assert "ssim" in [l.name for l in sr_amd.EDSR(scale_factor=2, n_feats=16, n_resblocks=1, losses=losses)._losses]


def test_ops_reexports():
    import sr_amd
    for name in ("ssim_torch", "SSIMLossFn", "ssim_loss"):
        assert hasattr(sr_amd.ops, name), name
    assert sr_amd.ops.ssim.__module__.endswith("ops_metrics"), "ops.ssim stays the metric"


# ---- clamp and pooling ----------------------------------------------------------------------------------------------------------
def test_gradient_is_zero_outside_the_unit_range_and_passes_on_its_ends(SL):
    sr, hr = REF.images((1, 3, 24, 24), 25)
    sr[0, 0, 12, 12], sr[0, 1, 12, 13], sr[0, 2, 13, 12] = 0.0, 1.0, 0.0          # exactly on the ends of the closed interval
    s = sr.clone().requires_grad_(True)
    SL.ssim_loss(s, hr).backward()
    outside = (sr < 0) | (sr > 1)
    assert outside.sum() > 100
    assert float(s.grad[outside].abs().max()) == 0.0
    for p in ((0, 0, 12, 12), (0, 1, 12, 13), (0, 2, 13, 12)):
        assert float(s.grad[p]) != 0.0, p
    _, g64 = REF.loss_and_grad(sr, hr)
    assert float(g64[outside].abs().max()) == 0.0 and all(float(g64[p]) != 0.0 for p in ((0, 0, 12, 12), (0, 1, 12, 13), (0, 2, 13, 12)))


def test_dropped_remainder_rows_and_columns_get_no_gradient(SL):
    sr, hr = REF.images((1, 1, 385, 391), 26)               # f = 2: row 384 and column 390 fall off the pooled image
    s = sr.clone().requires_grad_(True)
    SL.ssim_loss(s, hr).backward()
    assert float(s.grad[..., 384:, :].abs().max()) == 0.0 and float(s.grad[..., :, 390:].abs().max()) == 0.0
    inside = s.grad[..., :384, :390]
    assert float(inside.abs().max()) > 0.0
    # the four pixels of a 2 x 2 block that the clamp passes share their pooled pixel's gradient
    blk = inside[0, 0, 100:102, 300:302]
    assert bool(((sr[0, 0, 100:102, 300:302] >= 0) & (sr[0, 0, 100:102, 300:302] <= 1)).all())
    assert float(blk.max() - blk.min()) <= 1e-6 * float(blk.abs().max())


# ---- degenerate and refused inputs ---------------------------------------------------------------------------------------------
def test_identical_images(SL):
    _, hr = REF.images((2, 3, 32, 32), 27)
    s = hr.clone().requires_grad_(True)
    loss = SL.ssim_loss(s, hr)
    loss.backward()
    assert abs(float(loss.detach())) <= 1e-6
    assert torch.isfinite(s.grad).all()
    assert abs(float(REF.ssim_loss(hr, hr))) <= 1e-12


@pytest.mark.parametrize("hw", [(10, 32), (32, 10), (8, 8)])
def test_small_images_raise(SL, hw):
    x = torch.rand(1, 3, *hw)
    with pytest.raises(ValueError):
        SL.ssim_torch(x, x)
    with pytest.raises(ValueError):
        SL.ssim_loss(x, x)


def test_mismatched_shapes_raise(SL):
    with pytest.raises(ValueError):
        SL.ssim_loss(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17))
    with pytest.raises(ValueError):
        SL.ssim_loss(torch.rand(3, 16, 16), torch.rand(3, 16, 16))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_ssim_loss_args_mirror_the_header():
    import sr_amd
    assert sr_amd._lib.STRUCTS["srk_ssim_loss_args"] is sr_amd._lib.SsimLossArgs       # its layout: tests/test_host_surface.py
    assert {"srk_ssim_loss_fwd", "srk_ssim_loss_finalize", "srk_ssim_loss_bwd"} <= set(sr_amd._lib.LAUNCHERS)
    assert all(sr_amd._lib.LAUNCHERS["srk_ssim_loss_" + k] is sr_amd._lib.SsimLossArgs for k in ("fwd", "finalize", "bwd"))


def test_tile_count_and_refusals_of_the_library():
    """srk_ssim_loss_tiles is host code: the pooling factor is Python's round (halves to the even neighbour), the map is tiled 16 x 16,
    and what cannot run is refused with -1."""
    import sr_amd
    tiles = sr_amd._lib.load().srk_ssim_loss_tiles
    assert tiles(1, 3, 11, 11) == 3 and tiles(1, 1, 26, 26) == 1 and tiles(1, 1, 27, 27) == 4 and tiles(16, 3, 192, 192) == 48 * 144
    assert tiles(1, 1, 384, 391) == 12 * 12                 # f = 2 (1.5 rounds to 2): 192 x 195 pooled
    assert tiles(1, 1, 640, 640) == 20 * 20                 # f = 2 (2.5 rounds to 2): 320 x 320 pooled
    assert tiles(1, 1, 641, 644) == 13 * 13                 # f = 3: 213 x 214 pooled
    assert tiles(1, 1, 128, 128) == 8 * 8                   # f = 1 (0.5 rounds to 0, at least 1)
    assert tiles(65535, 1, 11, 11) == 65535 and tiles(21846, 3, 11, 11) == 65538
    assert tiles(1, 1, 10, 64) == -1 and tiles(1, 1, 64, 10) == -1 and tiles(0, 3, 32, 32) == -1
    assert tiles(1 << 24, 3, 192, 192) == -1                # planes x tiles past 2^31


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_train_py_ssim_composite_on_the_cpu():
    r = subprocess.run([sys.executable, "train.py", "-m", "srcnn", "--accelerator", "cpu", "--losses", "0.5*l1+0.5*ssim",
                        "--max_steps", "3", "--batch_size", "2", "--patch_size", "48", "--log_every", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    last = [l for l in r.stdout.splitlines() if l.startswith("done:")]
    assert last, r.stdout[-2000:]
    assert np.isfinite(float(last[0].split()[-1]))
