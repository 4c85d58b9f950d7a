"""CPU tests of gradient clipping (sr_amd.grad_clip): the float64 restatement of tests/clip_ref.py against torch.nn.utils' functions,
`GradClip` on CPU parameters under each of the four optimizers, the constructor's refusals, the model's and train.py's keywords, the
state dict, and the C ABI as the binding derives it from include/srk.h."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import sr_amd
from sr_amd.grad_clip import GradClip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R  # noqa: E402

SHAPES = [(7,), (3, 5, 3, 3), (4101,), (2, 4096)]           # 20,545 elements: fewer than 2^15 terms per sum
REL = 1e-10     # both sides are float64 sums of fewer than 2^15 terms (error <= 2^15 * 2^-53 = 3.6e-12 relative)
OPTIMIZERS = [("Adam", dict()), ("Ranger", dict(k=2)), ("SGD", dict(momentum=0.9, nesterov=True)), ("RMSprop", dict(centered=True, momentum=0.5))]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.rand(*s, generator=g) - 0.5) for s in SHAPES]


def _grads(step, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 + step)
    return [((torch.rand(*s, generator=g, dtype=dtype) - 0.5) * 10.0 ** (i % 3 - 1)) for i, s in enumerate(SHAPES)]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- the reference against torch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0.25, 2.0], ids=["clips", "does-not-clip"])
def test_reference_norm_is_torchs(factor):
    gs = _grads(0, torch.float64)
    norm = R.total_norm([g.numpy() for g in gs])
    max_norm = factor * norm
    want, n, c = R.clip_by_norm([g.numpy() for g in gs], max_norm)
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    tn = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    assert _rel(n, tn) <= REL and n == norm
    assert c == (1.0 if factor > 1 else R.coef(norm, max_norm)) and (c < 1.0) == (factor < 1)
    worst = 0.0
    for p, w in zip(ps, want):
        scale = float(np.abs(w).max())
        worst = max(worst, float(np.abs(p.grad.numpy() - w).max()) / scale)
    print(f"reference against torch (float64): norm rel {_rel(n, tn):.3g}, clipped elements rel-to-max {worst:.3g}")
    assert worst <= REL
    if factor < 1:
        assert _rel(R.total_norm(want), max_norm) <= 1e-6, "the clipped norm is max_norm (up to torch's 1e-6 in the denominator)"


def test_reference_value_clamp_is_torchs_and_keeps_nan():
    gs = _grads(1, torch.float64)
    gs[1].view(-1)[3] = float("nan")
    gs[2][5], gs[2][6] = float("inf"), float("-inf")
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    torch.nn.utils.clip_grad_value_(ps, 0.03)
    want = R.clip_by_value([g.numpy() for g in gs], 0.03)
    for p, w in zip(ps, want):
        assert np.array_equal(p.grad.numpy(), w, equal_nan=True)
    assert math.isnan(want[1].reshape(-1)[3]) and want[2][5] == 0.03 and want[2][6] == -0.03
    assert any(float(np.nanmax(np.abs(g.numpy()))) > 0.03 for g in gs) and all(float(np.nanmax(np.abs(w))) <= 0.03 for w in want)


# ---- GradClip on CPU parameters ------------------------------------------------------------------------------------------------------
def _make(name, kw, ps, ours=True):
    cls = getattr(sr_amd.optim if ours or name == "Ranger" else torch.optim, name)       # (torch has no Ranger: the package's own CPU form)
    return cls([{"params": ps[:2], "lr": 2e-3}, {"params": ps[2:], "lr": 1e-3}], **kw)


@pytest.mark.parametrize("algorithm,val", [("norm", 0.5), ("norm", 1e4), ("value", 0.02)], ids=["norm-clips", "norm-passes", "value"])
@pytest.mark.parametrize("name,kw", OPTIMIZERS, ids=[o[0] for o in OPTIMIZERS])
def test_cpu_parameters_take_torchs_clip_then_the_step(name, kw, algorithm, val):
    pa, pb = _params(1), _params(1)
    oa, ob = _make(name, kw, pa), _make(name, kw, pb, ours=False)
    clip = GradClip(oa, val, algorithm)
    assert oa._clip is clip and not clip.on_gpu
    for t in range(3):
        for p, q, g in zip(pa, pb, _grads(t)):
            p.grad, q.grad = g.clone(), g.clone()
        if t == 1:
            pa[1].grad = pb[1].grad = None                                    # a parameter without a gradient at one step
        oa.step()
        if algorithm == "norm":
            norm = torch.nn.utils.clip_grad_norm_(pb, val)
        else:
            torch.nn.utils.clip_grad_value_(pb, val)
        ob.step()
        for p, q in zip(pa, pb):
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), "p.grad holds the clipped gradient"
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach())
    if algorithm == "norm":
        s = clip.stats()
        assert s["total_norm"] == float(norm.float()) and s["num_nonfinite"] == 0
        assert s["num_clipped"] == (3 if val < 1 else 0) and (s["coef"] < 1.0) == (val < 1)
    clip.detach()
    assert oa._clip is None


def test_cpu_closure_runs_before_the_clip():
    ps = _params(2)
    opt = _make("SGD", {}, ps)
    GradClip(opt, 1e-3)

    def closure():
        for p, g in zip(ps, _grads(0)):
            p.grad = g.clone()
        return torch.tensor(1.5)
    assert float(opt.step(closure)) == 1.5
    assert R.total_norm([p.grad.numpy() for p in ps]) <= 1e-3 * (1 + 1e-6)


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("val,algorithm,err", [
    (0.0, "norm", ValueError), (-1.0, "norm", ValueError), (float("nan"), "value", ValueError), (float("inf"), "norm", ValueError),
    ("1", "norm", ValueError), (None, "norm", ValueError), (1.0, "l2", ValueError), (1.0, None, ValueError)])
def test_constructor_rejections(val, algorithm, err):
    opt = _make("Adam", {}, _params(3))
    with pytest.raises(err):
        GradClip(opt, val, algorithm)
    assert opt._clip is None, "nothing stays attached"


def test_unsupported_arguments_and_foreign_optimizers():
    ps = _params(3)
    opt = _make("Adam", {}, ps)
    with pytest.raises(NotImplementedError, match="norm_type"):
        GradClip(opt, 1.0, norm_type=1)
    with pytest.raises(NotImplementedError, match="norm_type"):
        GradClip(opt, 1.0, norm_type=float("inf"))
    with pytest.raises(NotImplementedError, match="foreach"):
        GradClip(opt, 1.0, foreach=True)
    with pytest.raises(TypeError, match="sr_amd.optim"):
        GradClip(torch.optim.Adam(ps), 1.0)
    assert opt._clip is None
    clip = GradClip(opt, 1.0)
    with pytest.raises(RuntimeError, match="already has"):
        GradClip(opt, 2.0)
    with pytest.raises(ValueError):
        clip.set_clip_val(0)
    clip.set_clip_val(3)
    assert clip.clip_val == 3.0 and float(clip.state[sr_amd._lib.SRK_CLIP_MAX_NORM]) == 3.0
    assert clip.total_norm.dim() == 0 and clip.coef.dim() == 0 and float(clip.coef) == 1.0
    assert sr_amd.optim._TableStep._clip is None and "_clip" not in vars(_make("SGD", {}, _params(4))), "a class-level default"


def test_state_dict_round_trip():
    pa = _params(5)
    oa = _make("SGD", {}, pa)
    ca = GradClip(oa, 0.5, "norm")
    for t in range(2):
        for p, g in zip(pa, _grads(t)):
            p.grad = g.clone()
        oa.step()
    sd = ca.state_dict()
    assert sd == dict(algorithm="norm", clip_val=0.5, num_clipped=2, num_nonfinite=0)
    cb = GradClip(_make("SGD", {}, _params(5)), 7.0, "value")
    cb.load_state_dict(sd)
    assert cb.state_dict() == sd and cb.algorithm == "norm" and cb.clip_val == 0.5
    L = sr_amd._lib
    assert float(cb.state[L.SRK_CLIP_MAX_NORM]) == 0.5 and float(cb.state[L.SRK_CLIP_CLIP_VALUE]) == 0.0
    with pytest.raises(ValueError):
        cb.load_state_dict(dict(sd, algorithm="l1"))


def test_srmodel_attaches_the_clipper_to_its_optimizer():
    opt = sr_amd.SRCNN(scale_factor=2, gradient_clip_val=0.5).configure_optimizers()[0]
    assert isinstance(opt._clip, GradClip) and opt._clip.clip_val == 0.5 and opt._clip.algorithm == "norm"
    opt = sr_amd.SRCNN(scale_factor=2, gradient_clip_val=2, gradient_clip_algorithm="value").configure_optimizers()[0]
    assert opt._clip.clip_val == 2.0 and opt._clip.algorithm == "value"
    assert sr_amd.SRCNN(scale_factor=2).configure_optimizers()[0]._clip is None
    assert sr_amd.SRCNN(scale_factor=2, gradient_clip_algorithm="value").configure_optimizers()[0]._clip is None, "no value: off"
    m = sr_amd.SRCNN(scale_factor=2, gradient_clip_val=0.5)
    m.grad_clip_state = dict(algorithm="norm", clip_val=0.25, num_clipped=9, num_nonfinite=1)
    assert m.configure_optimizers()[0]._clip.state_dict() == m.grad_clip_state
    for kw in (dict(gradient_clip_val=0), dict(gradient_clip_val=-1.0), dict(gradient_clip_val=1.0, gradient_clip_algorithm="l2"),
               dict(gradient_clip_algorithm="l2")):
        with pytest.raises(ValueError):
            sr_amd.SRCNN(scale_factor=2, **kw)


def test_train_py_saves_and_restores_the_clipper(tmp_path, capsys):
    """The CPU plumbing case: two steps that clip, --save, then two more from the checkpoint: the counter goes on from 2."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(root, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    common = ["-m", "srcnn", "--accelerator", "cpu", "--max_steps", "2", "--batch_size", "2", "--patch_size", "16", "-s", "2", "--precision", "32",
              "--log_every", "1", "--gradient_clip_val", "1e-6"]
    first, second = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    train.main(common + ["--save", first])
    assert torch.load(first, map_location="cpu")["grad_clip"] == dict(algorithm="norm", clip_val=1e-6, num_clipped=2, num_nonfinite=0)
    assert "grad norm" in capsys.readouterr().out
    train.main(common + ["--checkpoint", first, "--save", second])
    assert torch.load(second, map_location="cpu")["grad_clip"]["num_clipped"] == 4
    train.main(common[:-2] + ["--gradient_clip_val", "0.01", "--gradient_clip_algorithm", "value", "--save", second])
    assert torch.load(second, map_location="cpu")["grad_clip"] == dict(algorithm="value", clip_val=0.01, num_clipped=0, num_nonfinite=0)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_grad_clip_args_mirror_the_header():
    """The struct, the four launchers and the state indices as sr_amd._lib derives them from include/srk.h; every entry point checks
    its arguments before it launches anything (no GPU is touched: every call here is refused)."""
    L = sr_amd._lib
    lib = L.load()
    names = ("srk_grad_sumsq", "srk_grad_clip_coef", "srk_grad_clip_apply", "srk_grad_clip_value")
    for n in names:
        assert L.LAUNCHERS[n] is L.GradClipArgs is L.STRUCTS["srk_grad_clip_args"], n
        assert L.PROTOTYPES[n] == (ctypes.c_int, [ctypes.POINTER(L.GradClipArgs), ctypes.c_void_p]), n
    p, i = ctypes.c_void_p, ctypes.c_int
    assert L.GradClipArgs._fields_ == [("slots", p), ("blocks", p), ("nslots", i), ("nblocks", i), ("state", p), ("partials", p), ("base", i),
                                       ("nblocks_total", i), ("scaler_state", p)]
    assert [f for f, _ in L.GradClipArgs._fields_[:4]] == [f for f, _ in L.EmaArgs._fields_[:4]], "the table fields every table kernel starts with"
    assert (L.SRK_CLIP_MAX_NORM, L.SRK_CLIP_CLIP_VALUE, L.SRK_CLIP_TOTAL_NORM, L.SRK_CLIP_COEF, L.SRK_CLIP_NUM_CLIPPED,
            L.SRK_CLIP_NUM_NONFINITE) == (0, 1, 2, 3, 4, 5) and L.SRK_CLIP_STATE_FLOATS == 8

    def refused(name, msg, **kw):
        base = dict(slots=16, blocks=16, nslots=1, nblocks=2, state=16, partials=16, base=0, nblocks_total=2)      # (never dereferenced)
        base.update(kw)
        assert getattr(lib, name)(ctypes.byref(L.GradClipArgs(**base)), None) == L.SRK_E_BADARG, (name, kw)
        assert msg in lib.srk_last_error(), (name, kw, lib.srk_last_error())
    for n in ("srk_grad_sumsq", "srk_grad_clip_apply", "srk_grad_clip_value"):
        refused(n, b"null", slots=None)
        refused(n, b"null", state=None)
        refused(n, b"0 blocks", nblocks=0)
    refused("srk_grad_sumsq", b"partials", partials=None)
    refused("srk_grad_sumsq", b"of 2 partials", base=1)
    refused("srk_grad_sumsq", b"of 2 partials", base=-1)
    refused("srk_grad_clip_coef", b"null", partials=None)
    refused("srk_grad_clip_coef", b"0 partials", nblocks_total=0)
