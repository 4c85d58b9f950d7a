"""Whole images at batch 1 through `predict_step` / `validation_step` of every model with a HIP path, against the float64 oracle
(tests/eval_ref.py: reference, cases, limits; tests/test_eval_ref_cpu.py: what the limits rest on).

The sizes sit on either side of the thresholds the evaluation forward routes by -- ops.pair_ok (one-launch conv pair vs
weight-stationary / conv_ks), ops.hr_tail_ok (collapsed 5x5 HR stage), ops.rcab_chain's lazy channel attention, srk_ca_splits
(RCAN's global pool), the ragged conv_ks launch of 256 features -- and every case asserts its side through the project's own predicate
or counter, so a moved threshold cannot silently turn a case into a repeat of its neighbour.

Modes: precision 32 / 16 / 'bf16' as a user passes them (a bf16 model evaluates in fp16 storage, `SRModel.eval_dtype`, is judged as
fp16 and must be bit-identical to the fp16 model's image), and 'bf16' with eval_precision='bf16' for real bf16 storage.
Every case prints `EVAL ...` lines: measured value next to limit (run with -s to keep them)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_ref as ER  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["32", "16", "bf16", "bf16-storage"]
_DT = {"32": torch.float32, "16": torch.float16, "bf16": torch.bfloat16, "bf16-storage": torch.bfloat16}


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


@pytest.fixture(scope="module")
def cache(A):
    return ER.RefCache(A)


@pytest.mark.parametrize("case", ER.CASES, ids=lambda c: c.id)
@pytest.mark.parametrize("mode", MODES)
def test_whole_image_vs_float64_oracle(A, cache, case, mode):
    ref = cache.get(case)
    try:
        m, y = ER.compare_predict(A, ref, _DT[mode], eval_precision="bf16" if mode == "bf16-storage" else None)
        assert m.compute_dtype == _DT[mode]
        assert m.eval_dtype == {"32": torch.float32, "16": torch.float16, "bf16": torch.float16, "bf16-storage": torch.bfloat16}[mode]
        if mode == "bf16":
            # the substitution branch of SRModel._eval_forward: the image of the fp16 model holding the same weights, bit for bit
            m16 = ER.new_model(A, case, 16)
            m16.load_state_dict(ref.sd)
            y16 = ER.predict(m16.cuda().eval(), ref.x)
            assert torch.equal(y, y16), f"{case.id}: a bf16 model's predict_step differs from the fp16 model's " \
                                        f"(max |diff| {float((y - y16).abs().max()):.3e})"
        if case.val:
            ER.compare_validation(m, ref, y)
    finally:
        if mode == MODES[-1]:
            cache.drop(case)


def test_fp16_overflow_falls_back_to_training_dtype(A):
    """The other branch of SRModel._eval_forward: activations beyond fp16's 65504 (the preconditions are checked on the reference in
    test_eval_ref_cpu.py) make the fp16 evaluation forward non-finite, and a bf16 model's predict_step then returns its training
    dtype's image: finite, at the bf16 floor against the oracle, and the very image eval_precision='bf16' gives."""
    case = ER.OVERFLOW
    sd = ER.state_of(ER.new_model(A, case))
    ref = ER.Ref(case, sd, ER.image(3, case.h, case.w, ER.case_seed(case)))

    def on_gpu(precision, **extra):
        m = ER.new_model(A, case, precision, **extra)
        m.load_state_dict(sd)
        return m.cuda().eval()

    with torch.no_grad():
        y16 = on_gpu(16)(ref.x.cuda())
    assert not bool(torch.isfinite(y16).all()), "the fp16 forward stayed finite: the case does not reach the fallback"
    m = on_gpu("bf16")
    assert m.eval_dtype == torch.float16
    y = ER.predict(m, ref.x)
    ER.check_image(y, ref, torch.bfloat16, f"{case.id} precision=bf16 (fp16 overflow -> fallback)", u8=False)
    yb = ER.predict(on_gpu("bf16", eval_precision="bf16"), ref.x)
    assert torch.equal(y, yb)
