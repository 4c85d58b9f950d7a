"""CPU side of the D-DBPN whole-step tests (tests/ddbpn_ref.py, tests/test_gpu_ddbpn_step.py): what the GPU test's limits rest on is
established here, against the float64 oracle alone and without a GPU --

* the helper's restated loop IS the oracle's `ddbpn_forward`, and its hooked form (storage rounding / planted errors switched off) too;
* LIMIT32 (16 x the fp32-arithmetic baseline) is small enough to see one concatenation consumer's gradient of one slice counted twice;
* LIMIT16 (eval_ref.MARGIN x the storage-noise baseline) is small enough to see either gross wiring error in five tensors or more."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ddbpn_ref as DR  # noqa: E402
from oracle import functional as OF  # noqa: E402

NAME = {torch.float16: "fp16", torch.bfloat16: "bf16"}


@pytest.mark.parametrize("scale", DR.SCALES)
def test_restated_loop_is_the_oracle(scale):
    sd0, trainable, x, hr = DR.inputs(scale)
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    for k in trainable:
        sd[k].requires_grad_(True)
    y = OF.forward("DDBPN", sd, x.double(), scale_factor=scale)
    torch.nn.functional.l1_loss(y, hr.double()).backward()
    ref = DR.reference(scale)
    n, h, w = DR.LR_SHAPE[scale]
    assert tuple(ref["image"].shape) == (n, 3, h * scale, w * scale)
    assert torch.equal(ref["image"], y.detach())
    assert set(ref["grads"]) == set(trainable) and len(ref["parts"]) == 11
    for k in trainable:
        assert torch.equal(ref["grads"][k], sd[k].grad), k
    for k, g in ref["parts"].items():
        assert tuple(g.shape) == ((n, 32, h * scale, w * scale) if k[0] == "h" else (n, 32, h, w)), k
        assert float(g.abs().max()) > 0, k
    # the hooked units with every hook off (a planted error nothing consumes): the same arithmetic in the same order
    same = DR.run(scale, plant="slice", slice_plant=("none", 0))
    assert torch.equal(same["image"], ref["image"])
    for k in trainable:
        assert torch.equal(same["grads"][k], ref["grads"][k]), k
    for k in ref["parts"]:
        assert torch.equal(same["parts"][k], ref["parts"][k]), k


@pytest.mark.parametrize("scale", DR.SCALES)
def test_fp32_limit_sees_one_slice_counted_twice(scale):
    base, lim = DR.baseline32(scale), DR.limit32(scale)
    moves = DR.slice_movement(scale)
    print(f"D-DBPN x{scale}: fp32 baseline {base:.3e}, LIMIT32 {lim:.3e}, slice error moves its part by "
          + ", ".join(f"{p:.4f} (parameters {q:.4f})" for p, q in moves))
    assert 0 < base and lim <= 1e-3
    assert lim <= 0.25 * min(p for p, _ in moves)


@pytest.mark.parametrize("scale", DR.SCALES)
@pytest.mark.parametrize("dt", DR.DTYPES16, ids=lambda d: NAME[d])
def test_16bit_limit_sees_the_gross_errors(scale, dt):
    lim = DR.limit16(scale, dt)
    base = DR.baselines16(scale, dt)
    assert len(base) == (1 if scale == 4 else 2)
    assert lim == 2.0 * max(w for w, _ in base) and 0 < lim < 0.25
    for plant in ("double", "nosub"):
        sig = DR.gross_signature(scale, plant)
        count = sum(e > 2 * lim for e in sig)
        print(f"D-DBPN x{scale} {NAME[dt]}: LIMIT16 {lim:.4f}; '{plant}' moves {count} tensors by more than twice that (fifth largest {sig[4]:.3f})")
        assert count >= 5, f"'{plant}' would pass the 16-bit net: only {count} tensors above {2 * lim:.4f}"


def test_docstring_table_is_current():
    """The table in the helper's docstring is what `python tests/ddbpn_ref.py` prints (figures to 5 %: fp32 sums depend on the CPU)."""
    import re
    num = re.compile(r"(?<![A-Za-z_x])\d+\.?\d*(?:e-?\d+)?")
    now = DR.table().splitlines()
    doc = DR.__doc__.splitlines()
    start = doc.index(now[0])
    for a, b in zip(doc[start:start + len(now)], now, strict=True):
        assert num.sub("#", a).split() == num.sub("#", b).split(), (a, b)
        for u, v in zip(num.findall(a), num.findall(b), strict=True):
            u, v = float(u), float(v)
            assert abs(u - v) <= 0.05 * abs(v) + 1e-12 or (v < 1e-4 and 0.5 * v <= u <= 2 * v), (a, b)      # (fp32 figures: a factor 2)
