"""D-DBPN's whole training step (forward, L1, backward) at scales 2, 4 and 8 against the float64 oracle (tests/ddbpn_ref.py: reference
loop, cases, limits; tests/test_ddbpn_ref_cpu.py: what the limits rest on).

fp32 is the sharp instrument: the image within eval_ref.FP32_REL, every parameter gradient AND the gradient of each of the 11 parts of
the two concatenations (ops.SliceBuffer) within LIMIT32 = 16 x the CPU's fp32-arithmetic error -- a bound that one concatenation
consumer's gradient of one slice counted twice misses by a factor of 170 or more.  fp32 runs every projection on the im2col / col2im
column path at every scale.  bf16 / fp16 (loss scale 1024) is a net for gross wiring errors: PSNR floor, every sizeable parameter
gradient within LIMIT16 = eval_ref.MARGIN x the storage-noise model's worst tensor, and the shared gradient buffer of the concatenations
against autograd's own sums (`_SLICE_GACC` off).  Every limit is recomputed here from the helper's CPU runs.
Each case prints its worst observed ratio to the limit (run with -s to keep them)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ddbpn_ref as DR  # noqa: E402
import eval_ref as ER  # noqa: E402

pytestmark = pytest.mark.gpu

NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _step(A, monkeypatch, scale, dt):
    """One training step of the build on the case's inputs: dict(image, grads, parts, calls) on the CPU, gradients of the unscaled loss."""
    _, trainable, x, hr = DR.inputs(scale)
    calls, parts = {}, {}
    real_call, real_add = A._lib.call, A.ops.add_into

    def spy_call(name, args, stream):
        calls[name] = calls.get(name, 0) + 1
        return real_call(name, args, stream)

    def spy_add(a, b, dest):
        out = real_add(a, b, dest)
        if dest is not None:
            out.retain_grad()
            parts[("h" if dest[0].count == DR.DEPTH else "l") + str(dest[1])] = out
        return out

    with monkeypatch.context() as mp:
        mp.setattr(A._lib, "call", spy_call)
        mp.setattr(A.ops, "add_into", spy_add)
        torch.manual_seed(0)
        m = A.DDBPN(scale_factor=scale, precision=ER.PREC[dt]).cuda()
        assert m.compute_dtype == dt
        y = m(x.cuda())
        ls = 1.0 if dt == torch.float32 else DR.LOSS_SCALE
        (torch.nn.functional.l1_loss(y, hr.cuda()) * ls).backward()
        A.ops.flush_wgrads()
        torch.cuda.synchronize()
    assert tuple(parts) == tuple(sorted(parts, key=lambda k: (int(k[1:]), k[0] == "l"))) and set(parts) == set(DR.PART_NAMES), list(parts)
    params = dict(m.named_parameters())
    assert set(trainable) == {k for k, p in params.items() if p.requires_grad}
    return dict(image=y.detach().double().cpu(),
                grads={k: params[k].grad.detach().double().cpu() / ls for k in trainable},
                parts={k: p.grad.clone()[..., :32].permute(0, 3, 1, 2).double().cpu() / ls for k, p in parts.items()},
                calls=calls)


@pytest.mark.parametrize("scale", DR.SCALES)
def test_fp32_step_vs_float64_oracle(A, monkeypatch, scale):
    ref = DR.reference(scale)
    lim = DR.limit32(scale)
    got = _step(A, monkeypatch, scale, torch.float32)
    # fp32 storage: no direct projection kernels at any scale, 33 forward projections through unfold / fold
    assert got["calls"].get("srk_proj_up", 0) == 0 and got["calls"].get("srk_proj_down", 0) == 0 and got["calls"].get("srk_proj_wgrad", 0) == 0
    assert got["calls"].get("srk_unfold_nhwc", 0) >= 33 and got["calls"].get("srk_fold_nhwc", 0) >= 33, got["calls"]
    rel = float((got["image"] - ref["image"]).abs().max()) / max(1.0, float(ref["image"].abs().max()))
    err = DR.errors(got, ref)
    worst = max(err, key=err.get)
    print(f"DDBPN-STEP x{scale} fp32: image rel {rel:.2e} (< {ER.FP32_REL:.0e}); worst gradient {worst} {err[worst]:.3e} = "
          f"{err[worst] / lim:.3f} x LIMIT32 ({lim:.3e}); worst part {max((v, k) for k, v in err.items() if k.startswith('part:'))}")
    assert rel < ER.FP32_REL
    bad = {k: f"{v:.3e}" for k, v in err.items() if not v <= lim}
    assert not bad, f"x{scale} fp32: relative L2 above LIMIT32 = {lim:.3e}: {bad}"


@pytest.mark.parametrize("scale", DR.SCALES)
@pytest.mark.parametrize("dt", DR.DTYPES16, ids=lambda d: NAME[d])
def test_16bit_step_vs_float64_oracle(A, monkeypatch, scale, dt):
    ref = DR.reference(scale)
    lim = DR.limit16(scale, dt)
    got = _step(A, monkeypatch, scale, dt)
    direct = got["calls"].get("srk_proj_up", 0) + got["calls"].get("srk_proj_down", 0)
    if scale == 4:
        assert direct == 66 and got["calls"].get("srk_unfold_nhwc", 0) == 0 and got["calls"].get("srk_fold_nhwc", 0) == 0, got["calls"]
    else:
        assert direct == 0 and got["calls"].get("srk_unfold_nhwc", 0) >= 33 and got["calls"].get("srk_fold_nhwc", 0) >= 33, got["calls"]
    psnr = ER.psnr_db(got["image"], ref["image"])
    err = DR.errors(got, ref, parts=False, small=False)
    worst = max(err, key=err.get)
    # the shared gradient buffer against autograd's own sums of the slices
    monkeypatch.setattr(A.ops, "_SLICE_GACC", False)
    plain = _step(A, monkeypatch, scale, dt)
    ab = DR.errors(got, plain, parts=False, small=False)
    worst_ab = max(ab, key=ab.get)
    print(f"DDBPN-STEP x{scale} {NAME[dt]}: PSNR {psnr:.2f} dB (> {ER.PSNR_FLOOR[dt]}); worst gradient {worst} {err[worst]:.4f} = "
          f"{err[worst] / lim:.3f} x LIMIT16 ({lim:.4f}); against autograd's sums {worst_ab} {ab[worst_ab]:.4f} = {ab[worst_ab] / lim:.3f} x LIMIT16")
    assert psnr > ER.PSNR_FLOOR[dt]
    bad = {k: f"{v:.4f}" for k, v in err.items() if not v <= lim}
    assert not bad, f"x{scale} {NAME[dt]}: relative L2 above LIMIT16 = {lim:.4f}: {bad}"
    assert torch.equal(plain["image"], got["image"]), "the image changed with _SLICE_GACC off"
    bad = {k: f"{v:.4f}" for k, v in ab.items() if not v <= lim}
    assert not bad, f"x{scale} {NAME[dt]}: shared gradient buffer vs autograd's sums above LIMIT16 = {lim:.4f}: {bad}"
