"""MS-SSIM loss on the CPU: the float64 statement of tests/ms_ssim_loss_ref.py grounded on the metric's float64 statement
(tests/ms_ssim_ref.py) and on central differences, `ms_ssim_torch` in float64 and in fp32 against it (the calibration the GPU limits
rest on), the zero-gradient rule of a plane whose value is 0, the clamp, the loss string and its patch-size rule, the refused inputs,
the ctypes mirror of the header, the library's host-side geometry and train.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ms_ssim_loss_ref as REF  # noqa: E402
import ms_ssim_ref as METRIC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ML():
    from sr_amd import ms_ssim_loss
    return ms_ssim_loss


# ---- the reference is grounded ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 161, 176), (2, 3, 162, 161)], ids=["161x176", "162x161"])
def test_reference_value_is_one_minus_the_metric_statement(shape):
    sr, hr = REF.images(shape, 21)
    x = sr.clamp(0, 1).double()
    assert abs(float(REF.ms_ssim_loss(sr, hr)) - (1.0 - float(METRIC.ms_ssim(x, hr.double())["value"]))) <= 1e-12


def test_every_level_mean_of_the_test_inputs_is_well_above_zero():
    """On the `images` recipe no level mean comes near 0 (>= 0.55 in float64 on every shape of the list), so the zero-gradient rule
    hides nothing in the comparisons that use these inputs."""
    for shape in REF.SHAPES:
        sr, hr = REF.images(shape, 11 + sum(shape))
        assert float(REF.level_means(sr.clamp(0, 1), hr).min()) >= 0.55, shape


def test_reference_gradient_agrees_with_central_differences():
    """Central differences of the float64 loss, h = 1e-6, on (1, 1, 161, 176): H odd, so p = 1 pads the top and the left of level 0
    and the padded width 177 loses its last column, which is column 175 of the image.  Pixels: the corners, the edges, row 0 and
    column 0 (which carry the replicated pad's share), the dropped last column, interior pixels, the saturated corner of hr, and
    pixels inside both clamped regions (there the loss does not move at all and the gradient is exactly 0).

    The criterion of test_ssim_loss_cpu.py: 1e-6 relative, of the pixel's own gradient where that is large enough to be resolved,
    and never worse than 1e-6 of the largest gradient entry.  What the quotient itself resolves is coarser here than there: each loss
    is 1 - v with v near 0.9, so it carries a couple of ulps of 0.9 (1.1e-16 each), and the difference of two of them over 2h = 2e-6
    is good to about 4 * 2.2e-16 / 2e-6 = 4.4e-10 absolute, which is the floor under the relative test (the largest entry is 8e-4,
    so the floor is below 1e-6 of it)."""
    shape = (1, 1, 161, 176)
    sr, hr = REF.images(shape, 22)
    sr, hr = sr.double(), hr.double()
    _, g = REF.loss_and_grad(sr, hr)
    gmax = float(g.abs().max())
    h = 1e-6
    floor = 4 * np.finfo(np.float64).eps / (2 * h)
    assert floor < 1e-6 * gmax
    pixels = [(0, 0, 0, 0), (0, 0, 0, 175), (0, 0, 160, 0), (0, 0, 160, 175),                  # corners
              (0, 0, 0, 90), (0, 0, 0, 140), (0, 0, 80, 0), (0, 0, 120, 0), (0, 0, 160, 60),   # row 0, column 0, the last row
              (0, 0, 77, 175), (0, 0, 130, 175), (0, 0, 90, 174),                              # the dropped last column, and its neighbour
              (0, 0, 1, 1), (0, 0, 1, 0), (0, 0, 80, 100), (0, 0, 100, 81), (0, 0, 121, 133),  # interior
              (0, 0, 20, 20)]                                                                  # the saturated corner of hr
    above, below = torch.nonzero(sr > 1.0 + 1e-3), torch.nonzero(sr < -1e-3)                   # inside the clamped regions
    pixels += [tuple(int(i) for i in t[k]) for t in (above, below) for k in (len(t) // 3, 2 * len(t) // 3)]
    clamped = 0
    for p in pixels:
        v = float(sr[p])
        assert min(abs(v), abs(v - 1.0)) > 10 * h, "not on the clamp's kink"
        up, dn = sr.clone(), sr.clone()
        up[p] += h
        dn[p] -= h
        fd = (float(REF.ms_ssim_loss(up, hr)) - float(REF.ms_ssim_loss(dn, hr))) / (2 * h)
        got = float(g[p])
        if v < 0.0 or v > 1.0:
            clamped += 1
            assert fd == 0.0 and got == 0.0, (p, fd, got)
        else:
            assert abs(fd - got) <= max(1e-6 * abs(got), floor), (p, fd, got, gmax)
            assert abs(fd - got) <= 1e-6 * gmax
    assert 4 <= clamped <= 8


# ---- ms_ssim_torch against the reference ----------------------------------------------------------------------------------------
def test_float64_torch_statement_is_the_reference(ML):
    for shape in [(1, 1, 163, 209), (2, 3, 162, 161)]:
        sr, hr = REF.images(shape, 23)
        l64, g64 = REF.loss_and_grad(sr, hr)
        s = sr.double().requires_grad_(True)
        loss = ML.ms_ssim_loss(s, hr.double())
        loss.backward()
        assert abs(float(loss.detach()) - float(l64)) <= 1e-12
        assert float((s.grad - g64).abs().max()) <= 1e-10 * float(g64.abs().max())


@pytest.fixture(scope="module")
def calibration(ML):
    out = {}
    for shape in REF.SHAPES:
        sr, hr = REF.images(shape, 11 + sum(shape))
        l64, g64 = REF.loss_and_grad(sr, hr)
        s = sr.clone().requires_grad_(True)
        loss = ML.ms_ssim_loss(s, hr)
        loss.backward()
        out[shape] = REF.errors(loss.detach(), s.grad, l64, g64)
    return out


def test_fp32_torch_statement_leaves_the_gpu_limits_a_threefold_margin(calibration):
    """What fp32 arithmetic alone costs, on the GPU tests' own inputs and shapes.  Measured on the CPU over REF.SHAPES:
    |d loss| <= 2.4e-7, gradient relative L2 <= 1.1e-5, max error <= 4.0e-5 of the largest entry.  The limits the HIP path is given
    (REF.LIMIT_*) are the SSIM loss's own, 1e-5, 1e-3 and 3e-3: each is well over three times the value measured here, so they carry
    margin for the kernel's summation order over fp32 rounding itself, and none is looser than the single-scale loss's."""
    for shape, (dl, l2, worst) in calibration.items():
        print(f"\n{shape}: |dloss| {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert max(v[0] for v in calibration.values()) <= REF.LIMIT_LOSS / 3
    assert max(v[1] for v in calibration.values()) <= REF.LIMIT_L2 / 3
    assert max(v[2] for v in calibration.values()) <= REF.LIMIT_MAX / 3
    assert REF.LIMIT_LOSS <= 10 * 1e-5 and REF.LIMIT_L2 <= 10 * 1e-3 and REF.LIMIT_MAX <= 10 * 3e-3


# ---- the plane whose value is 0 ---------------------------------------------------------------------------------------------------
def test_anticorrelated_plane_gets_a_zero_gradient_and_the_others_keep_theirs(ML):
    sr, hr = REF.anticorrelated(0)
    m = REF.level_means(sr, hr)
    assert float(m[:, 0, 0].min()) <= 0.0, "a level mean of the anticorrelated plane is not positive in float64"
    assert float(m[:, 0, 1:].min()) > 0.5
    l64, g64 = REF.loss_and_grad(sr, hr)
    others = 1.0 - float(REF.ms_ssim_index(sr[:, 1:].clamp(0, 1), hr[:, 1:])) * 2.0 / 3.0
    assert abs(float(l64) - others) <= 1e-12, "the plane contributes v = 0"
    for dt in (torch.float32, torch.float64):
        s = sr.to(dt).clone().requires_grad_(True)
        loss = ML.ms_ssim_loss(s, hr.to(dt))
        loss.backward()
        assert abs(float(loss.detach()) - float(l64)) <= 1e-5
        assert torch.isfinite(s.grad).all()
        assert float(s.grad[0, 0].abs().max()) == 0.0
        assert float(s.grad[0, 1].abs().max()) > 0.0 and float(s.grad[0, 2].abs().max()) > 0.0
    assert torch.isfinite(g64).all() and float(g64[0, 0].abs().max()) == 0.0 and float(g64[0, 1].abs().max()) > 0.0


# ---- the clamp --------------------------------------------------------------------------------------------------------------------
def test_gradient_is_zero_outside_the_unit_range_and_passes_on_its_ends(ML):
    sr, hr = REF.images((1, 3, 161, 161), 25)
    ends = ((0, 0, 90, 90), (0, 1, 90, 91), (0, 2, 91, 90))
    sr[ends[0]], sr[ends[1]], sr[ends[2]] = 0.0, 1.0, 0.0          # exactly on the ends of the closed interval
    s = sr.clone().requires_grad_(True)
    ML.ms_ssim_loss(s, hr).backward()
    outside = (sr < 0) | (sr > 1)
    assert outside.sum() > 100
    assert float(s.grad[outside].abs().max()) == 0.0
    for p in ends:
        assert float(s.grad[p]) != 0.0, p
    _, g64 = REF.loss_and_grad(sr, hr)
    assert float(g64[outside].abs().max()) == 0.0 and all(float(g64[p]) != 0.0 for p in ends)


def test_identical_images(ML):
    _, hr = REF.images((1, 3, 161, 170), 27)
    s = hr.clone().requires_grad_(True)
    loss = ML.ms_ssim_loss(s, hr)
    loss.backward()
    assert abs(float(loss.detach())) <= 1e-6
    assert torch.isfinite(s.grad).all()
    assert abs(float(REF.ms_ssim_loss(hr, hr))) <= 1e-12


# ---- the loss string ------------------------------------------------------------------------------------------------------------
def test_model_accepts_the_l1_ms_ssim_composite():
    import sr_amd
    m = sr_amd.SRCNN(scale_factor=2, losses="0.16*l1+0.84*ms_ssim", patch_size=192)
    assert [(l.name, l.weight) for l in m._losses] == [("l1", 0.16), ("ms_ssim", 0.84)]
    sr, hr = REF.images((1, 3, 162, 161), 24)
    sr, hr = sr.float(), hr.float()
    out = m._calculate_losses(img_sr=sr, img_hr=hr)
    assert set(out) == {"loss", "loss/l1", "loss/ms_ssim"}
    want = 0.16 * float(torch.nn.functional.l1_loss(sr.double(), hr.double())) + 0.84 * float(REF.ms_ssim_loss(sr, hr))
    assert abs(float(out["loss"]) - want) <= 1e-5


def test_ms_ssim_in_the_loss_string_needs_a_patch_of_161():
    import sr_amd
    for losses in ("ms_ssim", "0.16*l1+0.84*ms_ssim", "l1 + 0.5*MS_SSIM"):
        with pytest.raises(ValueError, match="161"):
            sr_amd.SRCNN(scale_factor=2, losses=losses, patch_size=128)
        with pytest.raises(ValueError, match="161"):
            sr_amd.EDSR(scale_factor=2, n_feats=16, n_resblocks=1, losses=losses)            # the default patch is 128
        for patch in (161, 192):
            m = sr_amd.EDSR(scale_factor=2, n_feats=16, n_resblocks=1, losses=losses, patch_size=patch)
            assert "ms_ssim" in [l.name for l in m._losses]
    # every other loss string is what it was, whatever the patch
    assert [l.name for l in sr_amd.SRCNN(scale_factor=2, losses="0.16*l1+0.84*ssim", patch_size=48)._losses] == ["l1", "ssim"]


def test_ops_reexports():
    import sr_amd
    for name in ("ms_ssim_torch", "MSSSIMLossFn", "ms_ssim_loss"):
        assert hasattr(sr_amd.ops, name), name
    assert sr_amd.ops.ms_ssim.__module__.endswith("ops_metrics"), "ops.ms_ssim stays the metric"


# ---- refused inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(160, 192), (192, 160), (128, 128)])
def test_small_images_raise(ML, hw):
    x = torch.rand(1, 3, *hw)
    with pytest.raises(ValueError, match="161x161"):
        ML.ms_ssim_torch(x, x)
    with pytest.raises(ValueError, match="161x161"):
        ML.ms_ssim_loss(x, x)


def test_mismatched_shapes_raise(ML):
    with pytest.raises(ValueError):
        ML.ms_ssim_loss(torch.rand(1, 3, 161, 161), torch.rand(1, 3, 161, 162))
    with pytest.raises(ValueError):
        ML.ms_ssim_loss(torch.rand(3, 161, 161), torch.rand(3, 161, 161))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_ms_ssim_loss_args_mirror_the_header():
    import sr_amd
    assert sr_amd._lib.STRUCTS["srk_ms_ssim_loss_args"] is sr_amd._lib.MsSsimLossArgs       # its layout: tests/test_host_surface.py
    names = ["srk_ms_ssim_loss_" + k for k in ("fwd", "finalize", "bwd")]
    assert set(names) <= set(sr_amd._lib.LAUNCHERS)
    assert all(sr_amd._lib.LAUNCHERS[n] is sr_amd._lib.MsSsimLossArgs for n in names)
    assert {"srk_ms_ssim_loss_workspace_bytes", "srk_ms_ssim_loss_tiles"} <= set(sr_amd._lib.OTHER_SYMBOLS)


def test_tile_counts_workspace_and_refusals_of_the_library():
    """srk_ms_ssim_loss_tiles and srk_ms_ssim_loss_workspace_bytes are host code: the map tiling (16 x 16 over each level's valid map)
    and the pyramid are the metric's, and what cannot run is refused with -1."""
    import sr_amd
    lib = sr_amd._lib.load()
    first, mfirst = (ctypes.c_int * 6)(), (ctypes.c_int * 6)()
    # 161: levels 161, 81, 41, 21, 11 -> maps 151, 71, 31, 11, 1 -> 10^2, 5^2, 2^2, 1, 1 tiles
    assert lib.srk_ms_ssim_loss_tiles(1, 1, 161, 161, first) == 131 and list(first) == [0, 100, 125, 129, 130, 131]
    # 176: levels 176, 88, 44, 22, 11 -> maps 166, 78, 34, 12, 1 -> 11^2, 5^2, 3^2, 1, 1
    assert lib.srk_ms_ssim_loss_tiles(1, 1, 176, 176, first) == 157 and list(first) == [0, 121, 146, 155, 156, 157]
    # 192: levels 192, 96, 48, 24, 12 -> maps 182, 86, 38, 14, 2 -> 12^2, 6^2, 3^2, 1, 1
    assert lib.srk_ms_ssim_loss_tiles(16, 3, 192, 192, first) == 191 and list(first) == [0, 144, 180, 189, 190, 191]
    assert lib.srk_ms_ssim_loss_tiles(2, 3, 192, 192, None) == 191
    for n, c, h, w in [(1, 1, 161, 161), (1, 1, 176, 176), (16, 3, 192, 192), (2, 3, 162, 161), (1, 2, 161, 176), (1, 1, 163, 209)]:
        assert lib.srk_ms_ssim_loss_tiles(n, c, h, w, first) == lib.srk_ms_ssim_tiles(h, w, mfirst) and list(first) == list(mfirst)
        floats = 2 * n * c * sum(a * b for a, b in METRIC.pyramid_shapes(h, w)[1:])
        assert lib.srk_ms_ssim_loss_workspace_bytes(n, c, h, w) == (floats * 4 + 255) // 256 * 256
        assert lib.srk_ms_ssim_loss_workspace_bytes(n, c, h, w) == lib.srk_ms_ssim_workspace_bytes(n, c, h, w)
    assert lib.srk_ms_ssim_loss_tiles(70000, 1, 161, 161, None) == 131, "more planes than a 16-bit grid dimension"
    for bad in [(1, 1, 160, 192), (1, 1, 192, 160), (0, 3, 192, 192), (1, 0, 192, 192), (1, 1, 0, 0), (1 << 24, 3, 192, 192)]:
        assert lib.srk_ms_ssim_loss_tiles(*bad, None) == -1, bad
        assert lib.srk_ms_ssim_loss_workspace_bytes(*bad) == -1, bad


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_train_py_ms_ssim_composite_on_the_cpu():
    r = subprocess.run([sys.executable, "train.py", "-m", "srcnn", "--accelerator", "cpu", "--losses", "0.5*l1+0.5*ms_ssim",
                        "--patch_size", "176", "--batch_size", "2", "--max_steps", "2", "--log_every", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    last = [l for l in r.stdout.splitlines() if l.startswith("done:")]
    assert last, r.stdout[-2000:]
    assert np.isfinite(float(last[0].split()[-1]))
