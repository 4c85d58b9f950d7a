"""The pixel losses (Charbonnier, Huber, smooth-L1, robust, PSNR) on the CPU: the torch paths in float64 and fp32 against the float64
statement of tests/pixel_loss_ref.py, the fp32 floors the limits rest on, hand-checkable values, the loss string and `loss_params`
with their refusals, the re-exports and the ctypes mirror of the header."""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_loss_ref as REF  # noqa: E402

SHAPE_IDS = ["x".join(map(str, s)) for s in REF.SHAPES]
PSNR_IDS = ["x".join(map(str, s)) for s in REF.PSNR_SHAPES]
CASE_IDS = [c[0] for c in REF.CASES]


@pytest.fixture(scope="module")
def P():
    from sr_amd import pixel_loss
    return pixel_loss


@functools.lru_cache(maxsize=None)
def _images(shape, psnr=False):
    return (REF.psnr_images if psnr else REF.images)(shape, 11 + sum(shape))


@functools.lru_cache(maxsize=None)
def _case(cid, shape):
    """(sr, hr, float64 loss, float64 gradient) of one case and shape: computed once, read by every test that needs it."""
    if cid == "psnr":
        sr, hr = _images(shape, True)
        return (sr, hr) + REF.loss_and_grad("psnr", sr, hr, {})
    _, kind, params = REF.CASES[CASE_IDS.index(cid)]
    sr, hr = _images(shape)
    return (sr, hr) + REF.loss_and_grad(kind, sr, hr, params)


def _torch_loss_grad(P, kind, sr, hr, params):
    s = sr.clone().requires_grad_(True)
    loss = P.pixel_loss_torch(kind, s, hr, **params)
    loss.backward()
    return loss.detach(), s.grad


ALL = [(cid, kind, params, shape) for cid, kind, params in REF.CASES for shape in REF.SHAPES] + \
      [("psnr", "psnr", {}, shape) for shape in REF.PSNR_SHAPES]
ALL_IDS = [f"{cid}-{'x'.join(map(str, shape))}" for cid, _, _, shape in ALL]


# ---- the torch paths against the statement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,kind,params,shape", ALL, ids=ALL_IDS)
def test_torch_paths_against_the_statement(P, cid, kind, params, shape):
    """float64: the statement itself (1e-12); fp32: within the limits.  The gradient is exactly 0 where sr equals hr."""
    sr, hr, l64, g64 = _case(cid, shape)
    loss, g = _torch_loss_grad(P, kind, sr.double(), hr.double(), params)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and torch.isfinite(g64).all()
    assert max(REF.errors(loss, g, l64, g64)) <= 1e-12
    loss, g = _torch_loss_grad(P, kind, sr, hr, params)
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and torch.isfinite(g).all()
    assert dl <= REF.LIMIT_LOSS[kind] and l2 <= REF.LIMIT_L2[kind] and worst <= REF.LIMIT_MAX[kind], (dl, l2, worst)
    same = sr == hr
    if same.any():
        assert float(g[same].abs().max()) == 0.0 and float(g64[same].abs().max()) == 0.0


def test_inputs_carry_every_kind_of_difference():
    sr, hr = _images(REF.SHAPES[-1])
    d = (sr.double() - hr.double()).abs()
    n = d.numel()
    assert 0.10 < float((d == 0).sum()) / n < 0.15
    assert 0.2 < float(((d > 0) & (d < 1e-3)).sum()) / n < 0.3
    assert 0.005 < float((d > 1.4).sum()) / n < 0.015
    assert float((d == 0.5).sum()) / n > 0.015, "|d| exactly on the Huber / smooth-L1 threshold"
    assert float(sr.min()) < 0.0 and float(sr.max()) > 1.0, "nothing clamps"
    assert 0.0 <= float(hr.min()) and float(hr.max()) <= 1.0


def test_fp32_reference_statement_sets_the_limits():
    """The limits' calibration: the reference statement ITSELF in fp32 against itself in float64, per loss, the worst over its cases
    and shapes.  Measured: charbonnier 6.45e-08 5.89e-08 1.76e-07; huber and smooth_l1 1.10e-07 4.43e-08 3.82e-08; robust 1.61e-07
    5.11e-07 5.67e-07; psnr 8.32e-08 2.09e-07 2.26e-07 (loss, relative L2, max over largest).  The limits are ten times the floors
    written into pixel_loss_ref.py (at least three times what is measured here is asked for), and all stay fp32-sized."""
    worst = {}
    for cid, kind, params, shape in ALL:
        sr, hr, l64, g64 = _case(cid, shape)
        e = REF.errors(*REF.loss_and_grad(kind, sr, hr, params, torch.float32), l64, g64)
        worst[kind] = [max(a, b) for a, b in zip(worst.get(kind, (0.0, 0.0, 0.0)), e)]
    assert set(worst) == set(REF.FLOORS) == set(REF.LIMITS)
    for kind, got in worst.items():
        print(f"\n{kind}: floors {got[0]:.2e} {got[1]:.2e} {got[2]:.2e}")
        for g, floor, limit in zip(got, REF.FLOORS[kind], REF.LIMITS[kind]):
            assert g > 0.0
            assert 3 * g <= limit, "at least a threefold margin over what fp32 costs the statement itself"
            assert limit == 10.0 * floor and limit <= 1e-5


# ---- by hand ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_charbonnier_on_identical_images_is_eps_with_a_zero_gradient(P, dtype):
    _, hr = _images((2, 3, 16, 16))
    hr = hr.to(dtype)
    for eps in (1e-3, 1e-6):
        s = hr.clone().requires_grad_(True)
        loss = P.charbonnier_loss(s, hr, eps=eps)
        loss.backward()
        # fp32: the square, the root, the sum over 1,536 equal values and the division round a few times 6e-8
        assert abs(float(loss.detach()) - eps) <= (1e-6 if dtype == torch.float32 else 1e-15) * eps
        assert float(s.grad.abs().max()) == 0.0


def test_huber_and_smooth_l1_are_torchs(P):
    sr, hr = _images((1, 3, 5, 7))
    sr, hr = sr.double(), hr.double()
    for v in (0.5, 1.0, 0.05):
        assert abs(float(P.huber_loss(sr, hr, delta=v)) - float(F.huber_loss(sr, hr, delta=v))) <= 1e-15
        assert abs(float(P.smooth_l1_loss(sr, hr, beta=v)) - float(F.smooth_l1_loss(sr, hr, beta=v))) <= 1e-15
        assert abs(float(REF.huber(sr, hr, v)) - float(F.huber_loss(sr, hr, delta=v))) <= 1e-15
        assert abs(float(REF.smooth_l1(sr, hr, v)) - float(F.smooth_l1_loss(sr, hr, beta=v))) <= 1e-15
    assert float(P.huber_loss(sr, hr)) == float(P.huber_loss(sr, hr, delta=1.0)), "torch's default"
    assert float(P.smooth_l1_loss(sr, hr)) == float(P.smooth_l1_loss(sr, hr, beta=1.0))
    s = sr.clone().requires_grad_(True)
    loss = P.smooth_l1_loss(s, hr, beta=0.0)
    loss.backward()
    t = sr.clone().requires_grad_(True)
    F.l1_loss(t, hr).backward()
    assert float(loss.detach()) == float(F.l1_loss(sr, hr)) and torch.equal(s.grad, t.grad), "beta = 0 is L1"
    assert float(REF.smooth_l1(sr, hr, 0.0)) == float(F.l1_loss(sr, hr))


def test_robust_special_values(P):
    sr, hr = _images((2, 3, 16, 16))
    sr, hr = sr.double(), hr.double()
    d = sr - hr
    assert abs(float(P.robust_loss(sr, hr, alpha=2.0, c=1.0 / math.sqrt(2.0))) - float(F.mse_loss(sr, hr))) <= 1e-14
    for c in (0.01, 0.1):
        z = (d / c) ** 2
        want = float((torch.sqrt(z + 1.0) - 1.0).mean())
        assert abs(float(P.robust_loss(sr, hr, alpha=1.0, c=c)) - want) <= 1e-12 * want, "alpha = 1: sqrt(z + 1) - 1"
        assert abs(float(REF.robust(sr, hr, 1.0, c)) - want) <= 1e-12 * want
        want = float((2.0 * z / (z + 4.0)).mean())
        assert abs(float(P.robust_loss(sr, hr, alpha=-2.0, c=c)) - want) <= 1e-12 * want, "alpha = -2: Geman-McClure"


def test_robust_special_cases_are_continuous_in_alpha(P):
    """The general form tends to each exact case; the distance a neighbour at h keeps follows from expanding it, with |d| <= 0.3 and
    c = 0.1 (z <= 9):
      alpha = 2 - h   (h / (2 - h)) ((1 + z / h)^(1 - h / 2) - 1) = (z / 2) (1 - (h / 2) log(1 + z / h) + O(h)): relatively within
                      h (log(1 + 9 / h) / 2 + 1) = 5.6e-3 for h = 1e-3 (the h log h term: the family is continuous, not smooth, at 2);
      alpha = +-h     (b / 2) L + (b alpha / 8) L^2 + ..., L = log1p(z / b), b = 2 -+ h: within h (L / 4 + 1) <= 1.5e-3;
      alpha = -1e4    the exponent (alpha / 2) log1p(z / b) differs from -z / 2 by about (z + z^2 / 4) / |alpha| <= 30 / |alpha|.
    Each neighbour is another function: it does not coincide with the exact case to 1e-6."""
    g = torch.Generator().manual_seed(5)
    hr = torch.rand(1, 3, 32, 32, generator=g, dtype=torch.float64)
    sr = hr + 0.6 * (torch.rand(1, 3, 32, 32, generator=g, dtype=torch.float64) - 0.5)
    for exact, near, tol in ((2.0, 2.0 - 1e-3, 5.6e-3), (0.0, 1e-3, 1.5e-3), (0.0, -1e-3, 1.5e-3), (-math.inf, -1e4, 3e-3)):
        a, b = float(P.robust_loss(sr, hr, alpha=exact, c=0.1)), float(P.robust_loss(sr, hr, alpha=near, c=0.1))
        assert 1e-6 * abs(a) < abs(a - b) <= tol * abs(a), (exact, near, a, b)
        a, b = float(REF.robust(sr, hr, exact, 0.1)), float(REF.robust(sr, hr, near, 0.1))
        assert abs(a - b) <= tol * abs(a)


def test_psnr_loss_is_minus_the_psnr_metric(P):
    from sr_amd.models.srmodel import _psnr
    sr, hr = _images((2, 3, 16, 16))
    x = sr.clamp(0, 1)
    assert abs(float(P.psnr_loss(x, hr)) + float(_psnr(x, hr))) <= 1e-5 * abs(float(_psnr(x, hr)))
    assert abs(float(P.psnr_loss(x.double(), hr.double())) + float(_psnr(x, hr))) <= 1e-5 * abs(float(_psnr(x, hr)))
    assert abs(float(REF.psnr(x.double(), hr.double())) - float(P.psnr_loss(x.double(), hr.double()))) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_psnr_on_an_identical_pair_is_finite(P, dtype):
    _, hr = _images((2, 3, 16, 16))
    hr = hr.to(dtype)
    for eps in (1e-8, 1e-4):
        s = hr.clone().requires_grad_(True)
        loss = P.psnr_loss(s, hr, eps=eps)
        loss.backward()
        assert abs(float(loss.detach()) - 10.0 * math.log10(eps)) <= 1e-6 * abs(10.0 * math.log10(eps))
        assert float(s.grad.abs().max()) == 0.0


def test_mixed_and_half_dtypes_compute_in_fp32(P):
    sr, hr = _images((1, 3, 5, 7))
    want = float(REF.charbonnier(sr.double(), hr.double()))
    assert P.charbonnier_loss(sr.half(), hr).dtype == torch.float32
    # bf16 keeps 8 bits: each value (|sr| <= 2.5) moves by at most 2.5 * 2^-9, so |d| and with it the mean by at most 1e-2
    assert abs(float(P.charbonnier_loss(sr.bfloat16(), hr.bfloat16())) - want) <= 1e-2


# ---- the model --------------------------------------------------------------------------------------------------------------------
def test_model_trains_a_cpu_step_with_a_composite():
    import sr_amd
    m = sr_amd.SRCNN(scale_factor=2, losses="0.5*l1+0.5*charbonnier", loss_params=["charbonnier.eps=1e-6"])
    assert [(l.name, l.weight) for l in m._losses] == [("l1", 0.5), ("charbonnier", 0.5)]
    g = torch.Generator().manual_seed(0)
    lr, hr = torch.rand(2, 3, 12, 12, generator=g), torch.rand(2, 3, 24, 24, generator=g)
    out = m.training_step({"lr": lr, "hr": hr}, 0)
    assert set(out) == {"loss", "loss/l1", "loss/charbonnier"}
    sr = m(lr).detach()
    want_c = float(REF.charbonnier(sr.double(), hr.double(), eps=1e-6))
    assert abs(float(out["loss/charbonnier"].detach()) - 0.5 * want_c) <= 1e-6, "the weighted term, with the eps of loss_params"
    assert abs(want_c - float(REF.charbonnier(sr.double(), hr.double(), eps=1e-3))) > 1e-6
    assert abs(float(out["loss"].detach()) - 0.5 * float(F.l1_loss(sr, hr)) - 0.5 * want_c) <= 1e-6
    (opt,) = m.configure_optimizers()
    before = [p.detach().clone() for p in m.parameters()]
    out["loss"].backward()
    opt.step()
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))


@pytest.mark.parametrize("losses,params", [("charbonnier", []), ("huber", ["huber.delta=0.5"]), ("smooth_l1", ["smooth_l1.beta=0"]),
                                           ("robust", ["robust.alpha=-2", "robust.c=0.05"]), ("robust", ["robust.alpha=-inf", "robust.c=0.1"]),
                                           ("psnr", []), ("0.9*L1 + 0.1*PSNR", ["psnr.eps=1e-6"])])
def test_every_name_trains_on_the_cpu(losses, params):
    import sr_amd
    m = sr_amd.SRCNN(scale_factor=2, losses=losses, loss_params=params)
    g = torch.Generator().manual_seed(1)
    out = m.training_step({"lr": torch.rand(2, 3, 8, 8, generator=g), "hr": torch.rand(2, 3, 16, 16, generator=g)}, 0)
    out["loss"].backward()
    assert torch.isfinite(out["loss"]) and all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


@pytest.mark.parametrize("losses,params,match", [
    ("l1", ["charbonnier.eps=1e-6"], "not among the losses"),
    ("charbonnier", ["huber.delta=1"], "not among the losses"),
    ("l1", ["l1.eps=1"], "takes no parameters"),
    ("charbonnier", ["charbonnier.delta=1"], "no parameter delta"),
    ("charbonnier", ["charbonnier.eps=small"], "not a float"),
    ("charbonnier", ["charbonnier.eps"], "<loss>.<key>=<value>"),
    ("charbonnier", ["eps=1e-3"], "<loss>.<key>=<value>"),
    ("charbonnier", ["charbonnier.eps=0"], "out of range"),
    ("charbonnier", ["charbonnier.eps=-1e-3"], "out of range"),
    ("huber", ["huber.delta=0"], "out of range"),
    ("smooth_l1", ["smooth_l1.beta=-0.1"], "out of range"),
    ("psnr", ["psnr.eps=0"], "out of range"),
    ("robust", [], "alpha and c"),
    ("robust", ["robust.alpha=1"], "needs c"),
    ("robust", ["robust.c=0.1"], "needs alpha"),
    ("robust", ["robust.alpha=1", "robust.c=0"], "out of range"),
    ("robust", ["robust.alpha=inf", "robust.c=0.1"], "out of range"),
    ("robust", ["robust.alpha=nan", "robust.c=0.1"], "out of range"),
])
def test_loss_params_refusals(losses, params, match):
    import sr_amd
    with pytest.raises(ValueError, match=match):
        sr_amd.SRCNN(scale_factor=2, losses=losses, loss_params=params)


def test_entry_functions_refuse_bad_parameters(P):
    x = torch.rand(1, 3, 4, 4)
    for fn, kw in ((P.charbonnier_loss, dict(eps=0.0)), (P.huber_loss, dict(delta=-1.0)), (P.smooth_l1_loss, dict(beta=-1.0)),
                   (P.robust_loss, dict(alpha=math.inf, c=0.1)), (P.robust_loss, dict(alpha=float("nan"), c=0.1)),
                   (P.robust_loss, dict(alpha=1.0, c=0.0)), (P.psnr_loss, dict(eps=0.0))):
        with pytest.raises(ValueError):
            fn(x, x, **kw)
    with pytest.raises(TypeError):
        P.robust_loss(x, x)


def test_out_of_scope_losses_stay_out():
    import sr_amd
    for name in ("adaptive", "lpips", "0.5*l1+0.5*adaptive"):
        with pytest.raises(NotImplementedError):
            sr_amd.SRCNN(scale_factor=2, losses=name)
    with pytest.raises(AttributeError):
        sr_amd.SRCNN(scale_factor=2, losses="charbonier")


def test_train_py_takes_loss_params():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import train
    a = train.parse(["--losses", "0.5*l1+0.5*robust", "--loss_params", "robust.alpha=-2", "robust.c=0.05"])
    assert a.loss_params == ["robust.alpha=-2", "robust.c=0.05"] and train.parse([]).loss_params == []


# ---- ops, the C ABI ---------------------------------------------------------------------------------------------------------------
def test_ops_reexports():
    import sr_amd
    for name in ("pixel_loss_torch", "psnr_loss_torch", "PixelLossFn", "PSNRLossFn", "charbonnier_loss", "huber_loss", "smooth_l1_loss",
                 "robust_loss", "psnr_loss"):
        assert hasattr(sr_amd.ops, name), name


def test_args_mirror_the_header():
    import sr_amd
    L = sr_amd._lib
    assert L.STRUCTS["srk_pixel_loss_args"] is L.PixelLossArgs and L.STRUCTS["srk_psnr_loss_args"] is L.PsnrLossArgs
    assert all(L.LAUNCHERS["srk_pixel_loss_" + k] is L.PixelLossArgs for k in ("fwd", "bwd"))
    assert all(L.LAUNCHERS["srk_psnr_loss_" + k] is L.PsnrLossArgs for k in ("fwd", "finalize", "bwd"))
    assert "srk_pixel_loss_blocks" in L.OTHER_SYMBOLS and "srk_psnr_loss_blocks" in L.OTHER_SYMBOLS
    assert [L.SRK_PIXEL_CHARBONNIER, L.SRK_PIXEL_HUBER, L.SRK_PIXEL_SMOOTH_L1, L.SRK_PIXEL_ROBUST_A2, L.SRK_PIXEL_ROBUST_A0,
            L.SRK_PIXEL_ROBUST_NEG_INF, L.SRK_PIXEL_ROBUST_GENERAL] == list(range(7))
    assert (L.SRK_PIXEL_LOSS_BLOCK_ELEMS, L.SRK_PIXEL_LOSS_BLOCKS_MAX) == (REF.BLOCK_ELEMS, REF.BLOCKS_MAX)


def test_block_counts_of_the_library():
    """Host code: the elementwise grid is ceil(n / BLOCK_ELEMS) in [1, BLOCKS_MAX]; the PSNR grid is images x blocks per image, the
    latter capped so that the whole grid stays near BLOCKS_MAX, and what cannot run is refused with -1."""
    import sr_amd
    lib = sr_amd._lib.load()
    B, M = REF.BLOCK_ELEMS, REF.BLOCKS_MAX
    assert [lib.srk_pixel_loss_blocks(n) for n in (1, 3, B, B + 3, B + 4, B * M, B * M + 7, 1 << 33)] == [1, 1, 1, 1, 2, M, M, M]
    pb = lib.srk_psnr_loss_blocks
    assert pb(1, 1) == 1 and pb(3, 35) == 3 and pb(2, 768) == 2 and pb(65538, 4) == 65538 and pb(3, 1089) == 6
    assert pb(256, 3 * 192 * 192) == 256 * (M // 256) and pb(1, 1 << 40) == M
    assert pb(2, 257 * 259) == 2 * 66, "from 64 blocks per image on the finalize launch sums with a wave"
    assert pb(0, 4) == -1 and pb(4, 0) == -1 and pb(-1, 4) == -1
    assert pb(REF.PSNR_MOST_IMAGES, 1) == REF.PSNR_MOST_IMAGES and pb(REF.PSNR_MOST_IMAGES + 1, 1) == -1, "a grid below 2^32 threads"
    assert pb(1 << 20, 1 << 20) == 1 << 20 and pb((1 << 31) - 1, 4) == -1


def test_robust_kind_is_chosen_by_comparison(P):
    import sr_amd
    L = sr_amd._lib
    k = lambda a: P._kind_of("robust", {"alpha": a, "c": 0.1})[0]       # noqa: E731
    assert [k(2.0), k(0.0), k(-0.0), k(-math.inf)] == [L.SRK_PIXEL_ROBUST_A2, L.SRK_PIXEL_ROBUST_A0, L.SRK_PIXEL_ROBUST_A0, L.SRK_PIXEL_ROBUST_NEG_INF]
    assert all(k(a) == L.SRK_PIXEL_ROBUST_GENERAL for a in (2.0 - 1e-6, 1e-30, -1e-3, 1.0, -2.0, -1e30, 5.0, 2.0 ** -126))
    # the comparison is made on alpha as the launch carries it, in fp32
    for a, name in REF.EDGE_ALPHAS:
        got = P._kind_of("robust", {"alpha": a, "c": 0.1})
        assert (got is None) if name is None else (got[0] == getattr(L, "SRK_PIXEL_" + name)), (a, name)
    assert P._kind_of("robust", {"alpha": 2.0 - 1e-9, "c": 0.1})[1] == 2.0
    assert P._kind_of("robust", {"alpha": 1e39, "c": 0.1}) is None and P._kind_of("robust", {"alpha": 3e38, "c": 0.1}) is None


def test_parameters_fp32_cannot_hold_are_not_launched(P):
    """A constant the kernels derive (eps^2, delta / 2, beta / 2, c^2, 1 / c^2) that is zero, subnormal or infinite in fp32 keeps the
    parameter set off the HIP path; what is launched carries the fp32 value."""
    for kind, p in (("charbonnier", {"eps": 1e-20}), ("charbonnier", {"eps": 1e-50}), ("huber", {"delta": 1e-45}), ("huber", {"delta": 1e39}),
                    ("smooth_l1", {"beta": 1e-45}), ("robust", {"alpha": 1.0, "c": 1e-20}), ("robust", {"alpha": 1.0, "c": 1e20}),
                    ("robust", {"alpha": 2.0, "c": 1e-50})):
        assert P._kind_of(kind, p) is None, (kind, p)
    assert P._kind_of("charbonnier", {"eps": 1e-6})[1] == P._f32(1e-6) != 1e-6
    assert P._kind_of("smooth_l1", {"beta": 0.0}) is not None and P._kind_of("robust", {"alpha": 1.0, "c": 1e-18}) is not None


@pytest.mark.parametrize("alpha", [a for a, _ in REF.EDGE_ALPHAS], ids=lambda a: f"{a:g}")
def test_edge_alphas_on_the_torch_path(P, alpha):
    """fp32 inputs with an alpha at the edge of what fp32 holds: finite, and within the robust limits of the float64 statement at the
    alpha given (the fp32 path rounds alpha to fp32 or, where fp32 cannot hold it, computes in float64)."""
    sr, hr = _images((2, 3, 16, 16))
    params = {"alpha": alpha, "c": 0.1}
    l64, g64 = REF.loss_and_grad("robust", sr, hr, params)
    s = sr.clone().requires_grad_(True)
    loss = P.robust_loss(s, hr, **params)
    loss.backward()
    dl, l2, worst = REF.errors(loss.detach(), s.grad, l64, g64)
    assert loss.dtype == torch.float32 and torch.isfinite(loss) and torch.isfinite(s.grad).all() and torch.isfinite(g64).all()
    assert dl <= REF.LIMIT_LOSS["robust"] and l2 <= REF.LIMIT_L2["robust"] and worst <= REF.LIMIT_MAX["robust"], (dl, l2, worst)


def test_hip_entries_refuse_the_cpu(P):
    import sr_amd
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.PixelLossFn.apply(x, x, sr_amd._lib.SRK_PIXEL_CHARBONNIER, 1e-3, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.PSNRLossFn.apply(x, x, 1e-8)
