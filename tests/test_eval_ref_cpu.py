"""CPU side of the whole-image evaluation tests (tests/eval_ref.py, tests/test_gpu_eval_images.py): everything those tests take as given
is established here, against the float64 oracle alone and without a GPU --

* the baselines of the position checks are finite, and modest (row / column ratio < 3: the chosen input images do not by themselves
  make one row or column stand out);
* the uint8 contract's caps are CONDITIONS that each chosen input meets: the oracle with operands rounded to the storage dtype stays
  within them against the clean run;
* the preconditions of the fp16-overflow case hold on the reference;
* the position checks catch a wrong tile row that a PSNR floor lets through;
* the case list has both sides of every routing threshold and every model class the package exports (SRCNN has no HIP path)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_ref as ER  # noqa: E402
from oracle import functional as OF  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import sr_amd
    return sr_amd


@pytest.fixture(scope="module")
def cache(A):
    return ER.RefCache(A)


@pytest.mark.parametrize("case", ER.CASES, ids=lambda c: c.id)
def test_baselines_and_uint8_condition(cache, case):
    ref = cache.get(case)
    x = ref.x
    assert tuple(x.shape) == (1, case.channels, case.h, case.w) and float(x.min()) >= 0 and float(x.max()) <= 1
    assert float(x.std()) > 0.1, "the input needs structure"
    # enough of the reference image is not saturated: a clamped pixel has no error to profile.  (The nets without a MeanShift -- RDN,
    # SRResNet, single-channel EDSR -- centre their default-initialised image on 0, so about half of it clamps; the oracle runs and the
    # build clamp alike.)
    inside = float(((ref.ref > 0) & (ref.ref < 1)).double().mean())
    assert inside > 0.3, f"{case.id}: only {inside:.2f} of the reference image lies inside (0,1)"
    for dt in ER.DTYPES:
        b = ref.baseline(dt)
        print(f"BASE {case.id} {dt}: row {b['row']:.3f} col {b['col']:.3f} peak {b['peak']:.2f} PSNR {b['psnr']:.2f} dB "
              f"u8 max {b['u8max']} share {b['u8share']:.2e}")
        assert all(torch.isfinite(torch.tensor(float(v))) for v in b.values()), b
        assert b["row"] < ER.PROFILE_MAX and b["col"] < ER.PROFILE_MAX, f"{case.id} {dt}: badly chosen input image, {b}"
        assert b["row"] >= 1.0 and b["col"] >= 1.0 and b["peak"] >= 1.0
        if dt in ER.U8_SHARE:
            assert b["u8max"] <= 1 and b["u8share"] < ER.U8_SHARE[dt], f"{case.id} {dt}: the input does not meet the uint8 condition, {b}"
    # no case's floor comes from the operands-rounded oracle run: all are judged at the project's 50 / 62 dB (eval_ref.py docstring)
    for dt, floor in ER.PSNR_FLOOR.items():
        assert ref.floor(dt) == floor, f"{case.id} {dt}: operands-rounded oracle at {ref.baseline(dt)['psnr']:.2f} dB"
    cache.drop(case)


def test_overflow_case_preconditions(A):
    """The fallback branch of SRModel._eval_forward needs a net whose ACTIVATIONS leave fp16's range while its weights and its image do
    not: checked on the float64 reference."""
    case = ER.OVERFLOW
    m = ER.new_model(A, case)
    sd = ER.state_of(m)
    x = ER.image(3, case.h, case.w, ER.case_seed(case))
    for k, v in sd.items():
        assert bool(torch.isfinite(v.to(torch.float16)).all()), f"{k} itself overflows fp16"
    sd64 = {k: v.double() for k, v in sd.items()}
    head = OF.conv_same(sd64, "head.0", OF.mean_shift(sd64, "sub_mean", x.double()))
    assert float(head.abs().max()) > 65504.0, float(head.abs().max())
    assert float((head.abs() > 65504.0).double().mean()) > 0.01       # not one stray value: every image pixel has some within the trunk's reach
    y = ER.oracle(case, sd, x)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) < 4.0, float(y.abs().max())
    ref = ER.Ref(case, sd, x)
    b = ref.baseline(torch.bfloat16)
    print(f"BASE {case.id} bf16: {b}")
    assert ref.floor(torch.bfloat16) == ER.PSNR_FLOOR[torch.bfloat16]
    assert b["row"] < ER.PROFILE_MAX and b["col"] < ER.PROFILE_MAX


def test_position_checks_catch_what_psnr_misses(cache):
    """The last row of ONE 14x14 trunk tile (x4: 4 image rows x 56 columns) moved by 2^-10 -- the step of an fp16 activation between 1 and
    2 -- on an otherwise legitimate fp16-storage image: the row profile and the peak ratio exceed their limits, while the PSNR stays above
    the 62 dB floor, which is why the floors alone do not guard tile edges."""
    case = ER.BY_ID["edsr_x4_85x123"]
    ref = cache.get(case)
    dt = torch.float16
    base = ref.baseline(dt)
    y = ER.oracle(case, ref.sd, ref.x, dt).clamp(0, 1)
    row, col, peak = ER.local_stats(y - ref.ref)
    assert row < ER.MARGIN * base["row"] and col < ER.MARGIN * base["col"] and peak < ER.MARGIN * base["peak"]
    ty, tx, s = 2, 3, case.scale
    r0, c0 = (14 * ty + 13) * s, 14 * tx * s
    bad = y.clone()
    bad[..., r0:r0 + s, c0:c0 + 14 * s] += 2.0 ** -10
    row, col, peak = ER.local_stats(bad - ref.ref)
    print(f"corrupted tile row: row {row:.2f} (limit {ER.MARGIN * base['row']:.2f}), peak {peak:.2f} (limit {ER.MARGIN * base['peak']:.2f}), "
          f"PSNR {ER.psnr_db(bad, ref.ref):.2f} dB")
    assert row >= ER.MARGIN * base["row"], (row, base)
    assert peak >= ER.MARGIN * base["peak"], (peak, base)
    assert ER.psnr_db(bad, ref.ref) >= ref.floor(dt) == 62.0


def test_local_stats_on_known_errors():
    g = torch.Generator().manual_seed(0)
    e = torch.randn(1, 3, 200, 300, generator=g, dtype=torch.float64)
    row, col, peak = ER.local_stats(e)
    assert 1.0 < row < 1.3 and 1.0 < col < 1.3 and 4.0 < peak < 6.5
    e[..., 17, :] *= 3
    row2, col2, _ = ER.local_stats(e)
    assert 2.5 < row2 < 3.6 and abs(col2 - col) < 0.05
    shifted = ER.local_stats(e + torch.tensor([0.5, -2.0, 7.0], dtype=torch.float64).view(1, 3, 1, 1))     # a per-channel constant has no position
    assert all(abs(a - b) < 1e-9 for a, b in zip(shifted, ER.local_stats(e)))
    assert ER.u8_diff(torch.full((1, 1, 2, 2), 0.5), torch.full((1, 1, 2, 2), 0.5 + 1 / 255)) == (1, 1.0)


def test_case_list_covers_models_and_thresholds(A):
    classes = {c.cls for c in ER.CASES}
    exported = {n for n in ("EDSR", "RCAN", "RDN", "WDSR", "SRResNet", "DDBPN", "SRCNN") if hasattr(A, n)}
    assert classes == exported - {"SRCNN"}
    assert {c.cls for c in ER.CASES if c.val} == classes                      # one validation_step case per model
    scales = lambda cls: {c.scale for c in ER.CASES if c.cls == cls}          # noqa: E731
    assert scales("EDSR") >= {2, 3, 4} and scales("SRResNet") >= {2, 3, 4} and scales("DDBPN") == {2, 4, 8}
    assert {c.kw["rdn_config"] for c in ER.CASES if c.cls == "RDN"} == {"A", "B"}
    assert {c.kw["type"] for c in ER.CASES if c.cls == "WDSR"} == {"A", "B"}
    for cls, key in (("EDSR", "pair"), ("EDSR", "hr"), ("RCAN", "pair"), ("RCAN", "lazy"), ("RCAN", "hr")):
        assert {c.expect[key] for c in ER.CASES if c.cls == cls and key in c.expect} == {True, False}, (cls, key)
    # the thresholds themselves, through the library's host-side counters (no GPU needed for these two)
    lib = A._lib.load()
    by = ER.BY_ID
    assert lib.srk_conv_pair_tiles(1, 308, 322) == 506 and lib.srk_conv_pair_tiles(1, 309, 322) == 529
    assert lib.srk_conv_pair_tiles(1, 112, 112) == 64 and lib.srk_conv_pair_tiles(1, 113, 112) == 72
    for c in ER.CASES:
        if "splits" in c.expect:
            assert lib.srk_ca_splits(1, c.h * c.w) == c.expect["splits"], c.id
    sp = [by[i].expect["splits"] for i in ("rcan_248x264", "rcan_256x256", "rcan_256x257")]
    assert sp[0] < sp[1] == 1024 and sp[2] < 1024                             # below the cap, at it, past it (blocks of 65 pixels)
    # every DDBPN / x3 extent is odd or not a multiple of the stride / the 14- and 16-pixel tiles
    for c in ER.CASES:
        if c.cls == "DDBPN":
            assert c.h % 2 == 1 and c.w % 2 == 1 and c.h % c.scale and c.w % c.scale
    x3 = by["edsr_x3_47x173"]
    assert all(v % t for v in (x3.h, x3.w) for t in (14, 16))
