"""FLIP loss and metric on the CPU: the host tables and `flip_torch` against fixtures generated from the reference's own
losses/flip.py (tests/golden/generate_flip_golden.py), the model surface (`losses="flip"`, `metrics=["FLIP"]`) and train.py."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "flip_*.npz")))

# Tolerances, from the spread measured between flip_torch in fp32 and in float64 on these fixtures (both against the
# reference's fp32 result): loss <= 2.6e-7 relative; error map <= 5.5e-5 absolute (the saturated-plateau case: the clamp
# to the RGB box sits next to values that round either way; <= 9e-6 elsewhere); gradient <= 0.92 % of the largest
# reference gradient entry (plateau case again; <= 1.2e-3 relative elsewhere)
LOSS_RTOL = 1e-5
MAP_ATOL = 2e-4
GRAD_ATOL_REL = 2e-2


@pytest.fixture(scope="module")
def FL():
    import sr_amd
    return sr_amd.ops


def _load(path):
    return dict(np.load(path))


def test_fixtures_are_present():
    names = {os.path.basename(p) for p in FIXTURES}
    assert len(names) >= 6 and "flip_tiny_1x7x5.npz" in names and "flip_odd_1x85x123.npz" in names, names


def test_tables_match_the_reference_filters_bit_for_bit(FL):
    t = FL.flip_tables()
    z = _load(FIXTURES[0])
    for mine, ref in (("csf_a_2d", "csf_a"), ("csf_rg_2d", "csf_rg"), ("csf_by_2d", "csf_by"), ("edge_2d", "edge"), ("point_2d", "point")):
        assert t[mine].dtype == np.float32 and t[mine].shape == z[ref].shape
        assert np.array_equal(t[mine].view(np.uint32), z[ref].view(np.uint32)), mine
    assert t["cmax"] == float(z["cmax"])
    assert t["csf_radius"] == int(z["csf_radius"]) == 10 and t["feature_radius"] == 9
    assert t["ppd"] == float(z["ppd"])


def test_separable_taps_rebuild_the_2d_filters(FL):
    """The kernels filter with 1-D passes: the outer products equal the reference's 2-D filters up to fp32 rounding."""
    t = FL.flip_tables()
    outer = np.outer
    assert np.abs(outer(t["csf_a"], t["csf_a"]) - t["csf_a_2d"]).max() < 1e-7
    assert np.abs(outer(t["csf_rg"], t["csf_rg"]) - t["csf_rg_2d"]).max() < 1e-7
    by = t["by_w"][0] * outer(t["csf_by1"], t["csf_by1"]) + t["by_w"][1] * outer(t["csf_by2"], t["csf_by2"])
    assert np.abs(by - t["csf_by_2d"]).max() < 1e-7
    assert np.abs(outer(t["gauss"], t["edge"]) - t["edge_2d"]).max() < 1e-7
    assert np.abs(outer(t["gauss"], t["point"]) - t["point_2d"]).max() < 1e-7
    tab = t["table"]
    assert tab.dtype == np.float32 and tab.size == 176            # include/srk.h SRK_FLIP_TABLE_FLOATS


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[5:-4] for p in FIXTURES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_flip_torch_matches_the_reference(FL, path, dtype):
    z = _load(path)
    sr = torch.tensor(z["sr"], dtype=dtype, requires_grad=True)
    hr = torch.tensor(z["hr"], dtype=dtype)
    err = FL.flip_error_map_torch(sr, hr)
    loss = err.mean()
    loss.backward()
    ref_loss = float(z["loss"])
    assert abs(float(loss) - ref_loss) <= LOSS_RTOL * ref_loss, (float(loss), ref_loss)
    assert float(np.abs(err.detach().numpy()[:, 0] - z["err"]).max()) <= MAP_ATOL
    g, rg = sr.grad.numpy(), z["grad"]
    assert np.isfinite(g).all(), "the gradient is finite everywhere (the reference's is NaN where the colours coincide)"
    fin = np.isfinite(rg)
    assert fin.sum() > 0.4 * rg.size
    tol = GRAD_ATOL_REL * float(np.abs(rg[fin]).max())
    assert float(np.abs(g[fin] - rg[fin]).max()) <= tol, (float(np.abs(g[fin] - rg[fin]).max()), tol)


def test_zero_gradient_where_the_reference_is_nan(FL):
    """Columns 24.. where sr == hr: the reference's autograd gives NaN there, ours is finite, and 0 at least 20 columns into
    that half (every error pixel within the filters' reach has coinciding colours: a minimum of the error)."""
    z = _load(os.path.join(GOLDEN, "flip_halfequal_2x48x48.npz"))
    assert np.isnan(z["grad"][..., 24:]).all()
    sr = torch.tensor(z["sr"], requires_grad=True)
    FL.flip_torch(sr, torch.tensor(z["hr"])).backward()
    g = sr.grad.numpy()
    assert np.isfinite(g).all() and float(np.abs(g[..., 44:]).max()) == 0.0


def test_flip_loss_on_the_cpu_is_flip_torch(FL):
    z = _load(FIXTURES[0])
    sr, hr = torch.tensor(z["sr"]), torch.tensor(z["hr"])
    assert float(FL.flip_loss(sr, hr)) == float(FL.flip_torch(sr, hr))
    assert float(FL.flip(sr, hr)) == float(FL.flip_torch(sr, hr))
    assert FL.flip_error_map(sr, hr).shape == (2, 1, 48, 48)
    with pytest.raises(ValueError):
        FL.flip_torch(sr[:, :1], hr[:, :1])


def test_model_accepts_flip_loss_and_metric():
    import sr_amd
    for losses in ("flip", "0.8*l1+0.2*flip", "l1 + 0.5*FLIP"):
        m = sr_amd.SRCNN(scale_factor=2, losses=losses, metrics=["PSNR", "FLIP"])
        assert "flip" in [l.name for l in m._losses]
        assert "FLIP" in [n for n, _ in m._metrics]
    m = sr_amd.SRCNN(scale_factor=2, losses="0.8*l1+0.2*flip")
    assert [(l.name, l.weight) for l in m._losses] == [("l1", 0.8), ("flip", 0.2)]
    g = torch.Generator().manual_seed(0)
    lr, hr = torch.rand(2, 3, 12, 12, generator=g), torch.rand(2, 3, 24, 24, generator=g)
    out = m.training_step({"lr": lr, "hr": hr}, 0)
    out["loss"].backward()
    sr = m(lr).detach()
    want = 0.8 * torch.nn.functional.l1_loss(sr, hr) + 0.2 * sr_amd.ops.flip_torch(sr, hr)
    assert abs(float(out["loss"]) - float(want)) < 1e-6
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    m2 = sr_amd.SRCNN(scale_factor=2, metrics=["PSNR", "SSIM", "FLIP"], eval_datasets=["X"])
    res = m2.validation_step({"lr": lr, "hr": hr}, 0)
    assert abs(float(res["X/FLIP"]) - float(sr_amd.ops.flip_torch(m2(lr).clamp(0, 1), hr.clamp(0, 1)))) < 1e-6


@pytest.mark.parametrize("kw", [dict(losses="flip"), dict(metrics=["PSNR", "FLIP"]), dict(losses="l1+flip", metrics=["FLIP"])])
def test_flip_needs_three_channels(kw):
    import sr_amd
    with pytest.raises(ValueError, match="channels"):
        sr_amd.SRCNN(scale_factor=2, channels=1, **kw)


def test_train_py_flip_composite_on_the_cpu():
    r = subprocess.run([sys.executable, "train.py", "-m", "srcnn", "--accelerator", "cpu", "--losses", "0.5*l1+0.5*flip",
                        "--max_steps", "3", "--batch_size", "2", "--patch_size", "48", "--log_every", "1", "--metrics", "PSNR", "FLIP"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    last = [l for l in r.stdout.splitlines() if l.startswith("done:")]
    assert last, r.stdout[-2000:]
    assert np.isfinite(float(last[0].split()[-1]))
