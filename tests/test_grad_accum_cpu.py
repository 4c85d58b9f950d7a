"""CPU tests of gradient accumulation (sr_amd.grad_accum): the two rules against the float64 restatement of tests/grad_accum_ref.py and,
bit for bit, against its fp32 restatement; `Trainer.fit` with `accumulate_grad_batches` against Lightning's recipe written out by hand
(`loss / k`, autograd adding into `.grad`, torch's own optimizer step) on SRCNN; the step hooks (EMA, lr schedule, clipper) once per
window; the refusals; the model's and train.py's keywords; the C ABI as the binding derives it from include/srk.h; the documented table.

Tolerance of the float64 comparison: (k + 2) * 2^-24 * (sum_j |g_j|) / k per element -- k - 1 additions, the rounding of inv_k, one
multiplication, one unit of slack for second-order terms (grad_accum_ref.bound).  The inputs are drawn from +-[0.05, 1]: nothing is
subnormal."""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sr_amd
from sr_amd import trainer as T
from sr_amd.grad_accum import GradAccum, check_args

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_accum_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7,), (3, 5, 3, 3), (4101,)]
OPTIMIZERS = ["ADAM", "Ranger", "SGD", "RMSprop"]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.rand(*s, generator=g) - 0.5) for s in SHAPES]


def _grads(seed):
    """+-[0.05, 1]"""
    g = torch.Generator().manual_seed(5000 + seed)
    out = []
    for s in SHAPES:
        mag = 0.05 + 0.95 * torch.rand(*s, generator=g)
        sign = torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
        out.append((mag * sign).float().numpy())
    return out


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4, 7])
def test_rules_against_float64_and_the_fp32_restatement(k):
    ps = _params(0)
    opt = sr_amd.optim.SGD(ps, lr=1e-3)
    acc = GradAccum(opt, k)
    assert acc.inv_k == float(R.inv_k(k)) and not acc.on_gpu
    for window in range(2):                                  # the second window starts from the zeros FINAL left
        micro = [_grads(10 * window + j) for j in range(k)]
        for j in range(k):
            assert acc.phase == ("step" if j == k - 1 else "accumulate") and acc.pos == j
            for p, g in zip(ps, micro[j]):
                p.grad = torch.from_numpy(g.copy())
            assert acc.step() == (j == k - 1)
        assert acc.pos == 0
        worst = 0.0
        for i, p in enumerate(ps):
            per = [micro[j][i] for j in range(k)]
            got = p.grad.numpy()
            assert got.dtype == np.float32 and np.array_equal(got, R.window_f32(per)), "the pinned fp32 order, bit for bit"
            err, lim = np.abs(got.astype(np.float64) - R.window_f64(per)), R.bound(per)
            worst = max(worst, float((err / lim).max()))
            assert (err <= lim).all()
            assert float(np.abs(np.stack(per)).min()) >= 0.05
        print(f"k={k} window {window}: worst error / bound {worst:.3f}")
        for a in acc._acc.values():
            assert not a.any(), "FINAL zeroes acc"


# ---- Lightning parity ---------------------------------------------------------------------------------------------------------------
def _batches(k, windows=3):
    return [T.synthetic_batch(2, 3, 8, 2, 700 + i, "cpu") for i in range(windows * k)]


def _hand_loop(model, name, k, batches):
    """Lightning's recipe on a copy of the model: zero_grad; k times backward of loss / k (k = 3: backward of the loss, then one multiply
    by float32(1 / 3), the pinned rule); torch's own optimizer step (Ranger: the package's CPU form, torch has none)."""
    m = copy.deepcopy(model)
    cls = {"ADAM": torch.optim.Adam, "SGD": torch.optim.SGD, "RMSprop": torch.optim.RMSprop, "Ranger": sr_amd.optim.Ranger}[name]
    opt = cls([p for p in m.parameters() if p.requires_grad], **m._optim_params)
    for w in range(len(batches) // k):
        opt.zero_grad()
        for b in batches[w * k:(w + 1) * k]:
            loss = m._calculate_losses(img_sr=m(b["lr"]), img_hr=b["hr"])["loss"]
            (loss if k == 3 else loss / k).backward()
        if k == 3:
            for p in m.parameters():
                p.grad.mul_(float(np.float32(1.0 / 3.0)))
        opt.step()
    return m


@pytest.mark.parametrize("k", [2, 4, 3])
@pytest.mark.parametrize("name", OPTIMIZERS)
def test_fit_is_lightnings_accumulation_bit_for_bit(name, k):
    torch.manual_seed(0)
    model = sr_amd.SRCNN(scale_factor=2, optimizer=name, losses="l1", precision=32, accumulate_grad_batches=k)
    batches = _batches(k)
    h1, h2 = _hand_loop(model, name, k, batches), _hand_loop(model, name, k, batches)
    start = [p.detach().clone() for p in model.parameters()]
    for a, b in zip(h1.parameters(), h2.parameters()):
        assert torch.equal(a, b), "precondition: the hand loop is deterministic"
    tr = T.Trainer(device="cpu")
    tr.fit(model, batches)
    assert len(tr.losses) == 3 * k, "one loss per batch"
    assert isinstance(tr.optimizer._accum, GradAccum) and tr.optimizer._accum.pos == 0
    for p, q, s in zip(model.parameters(), h1.parameters(), start):
        assert torch.equal(p.detach(), q.detach())
        assert not torch.equal(p.detach(), s)


# ---- the step hooks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_hooks_run_once_per_window(k):
    n = 3
    torch.manual_seed(0)
    model = sr_amd.SRCNN(scale_factor=2, optimizer="ADAM", precision=32, accumulate_grad_batches=k, ema_decay=0.9, lr_schedule="step",
                         lr_schedule_params=["step_size=1", "gamma=0.5"], gradient_clip_val=1e-6)
    tr = T.Trainer(device="cpu")
    tr.fit(model, _batches(k, n) + _batches(k, 1)[:k - 1])     # n windows and an incomplete one, which is dropped
    opt = tr.optimizer
    assert model.ema.num_updates == n and opt.lr_schedule.count == n
    assert opt._clip.stats()["num_clipped"] == n, "the clipper saw one norm per window"
    assert opt.param_groups[0]["lr"] == 1e-3 * 0.5 ** n
    assert all(int(opt.state[p]["step"]) == n for p in model.parameters())
    assert len(tr.losses) == n * k + k - 1
    assert opt._accum.pos == 0 and all(not a.any() for a in opt._accum._acc.values()), "the incomplete window was dropped"


def test_max_steps_counts_optimizer_steps(capsys):
    torch.manual_seed(0)
    model = sr_amd.SRCNN(scale_factor=2, precision=32, accumulate_grad_batches=2, lr_schedule="constant")
    tr = T.Trainer(device="cpu", max_steps=2, log_every=1)
    tr.fit(model, _batches(2, 5))
    assert len(tr.losses) == 4 and tr.optimizer.lr_schedule.count == 2
    out = capsys.readouterr().out
    assert "step 1:" in out and "step 2:" in out and "step 3:" not in out


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, -1, 2.5, True, "2"])
def test_bad_window_lengths_are_refused(k):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        check_args(k)
    opt = sr_amd.optim.SGD(_params(1), lr=1e-3)
    with pytest.raises(ValueError):
        GradAccum(opt, k)
    assert opt._accum is None, "nothing stays attached"
    with pytest.raises(ValueError):
        sr_amd.SRCNN(scale_factor=2, accumulate_grad_batches=k)


def test_foreign_optimizers_and_double_attachment_are_refused():
    ps = _params(2)
    with pytest.raises(TypeError, match="sr_amd.optim"):
        GradAccum(torch.optim.SGD(ps, lr=1e-3), 2)
    opt = sr_amd.optim.Adam(ps)
    GradAccum(opt, 2)
    with pytest.raises(RuntimeError, match="already has"):
        GradAccum(opt, 3)
    with pytest.raises(RuntimeError, match="GradAccum"):
        sr_amd.optim.Adam(_params(2)).accumulate()


def test_a_gradient_missing_in_one_micro_step_raises():
    ps = _params(3)
    opt = sr_amd.optim.SGD(ps, lr=1e-3)
    acc = GradAccum(opt, 3)
    for p, g in zip(ps, _grads(0)):
        p.grad = torch.from_numpy(g)
    acc.step()
    ps[1].grad = None
    with pytest.raises(RuntimeError, match="set of tensors"):
        acc.step()
    acc.reset()
    assert acc.pos == 0 and acc.phase == "accumulate"
    with pytest.raises(RuntimeError, match="full"):
        for _ in range(3):
            opt.accumulate()


# ---- k = 1 and detach ---------------------------------------------------------------------------------------------------------------
def test_k_one_attaches_nothing_and_detach_restores_the_optimizer():
    assert sr_amd.SRCNN(scale_factor=2).configure_optimizers()[0]._accum is None
    assert sr_amd.SRCNN(scale_factor=2, accumulate_grad_batches=1).configure_optimizers()[0]._accum is None
    opt = sr_amd.SRCNN(scale_factor=2, accumulate_grad_batches=4).configure_optimizers()[0]
    assert isinstance(opt._accum, GradAccum) and opt._accum.k == 4 and opt._accum.phase == "accumulate"
    assert sr_amd.optim._TableStep._accum is None and "_accum" not in vars(sr_amd.optim.SGD(_params(4), lr=1e-3)), "a class-level default"
    pa, pb = _params(5), _params(5)
    oa, ob = sr_amd.optim.SGD(pa, lr=1e-2, momentum=0.9), torch.optim.SGD(pb, lr=1e-2, momentum=0.9)
    acc = GradAccum(oa, 2)
    acc.detach()
    acc.detach()
    assert oa._accum is None and acc.optimizer is None
    for t in range(2):
        for p, q, g in zip(pa, pb, _grads(t)):
            p.grad, q.grad = torch.from_numpy(g.copy()), torch.from_numpy(g.copy())
        oa.step()
        ob.step()
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach()), "a plain optimizer again: every call steps"


# ---- entry point, C ABI, documentation ----------------------------------------------------------------------------------------------
def _train_cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    return train


def test_train_py_takes_the_flag(tmp_path, capsys):
    train = _train_cli()
    assert train.parse([]).accumulate_grad_batches == 1
    assert train.parse(["--accumulate_grad_batches", "4"]).accumulate_grad_batches == 4
    with pytest.raises(SystemExit):
        train.main(["-m", "srcnn", "--accelerator", "cpu", "--accumulate_grad_batches", "0"])
    save = str(tmp_path / "a.pt")
    train.main(["-m", "srcnn", "--accelerator", "cpu", "--max_steps", "2", "--accumulate_grad_batches", "2", "--batch_size", "2", "--patch_size", "16",
                "-s", "2", "--precision", "32", "--log_every", "0", "--lr_schedule", "constant", "--ema_decay", "0.5", "--save", save])
    assert "done: 4 steps" in capsys.readouterr().out, "max_steps * K batches were consumed"
    sd = torch.load(save, map_location="cpu")
    assert sd["lr_schedule"]["count"] == 2 and sd["ema_num_updates"] == 2


def test_grad_accum_args_mirror_the_header():
    """The struct, the launcher and the two operations as sr_amd._lib derives them from include/srk.h; the entry point checks its
    arguments before it launches anything (no GPU is touched: every call here is refused)."""
    L = sr_amd._lib
    lib = L.load()
    assert L.LAUNCHERS["srk_grad_accum"] is L.GradAccumArgs is L.STRUCTS["srk_grad_accum_args"]
    assert L.PROTOTYPES["srk_grad_accum"] == (ctypes.c_int, [ctypes.POINTER(L.GradAccumArgs), ctypes.c_void_p])
    p, i = ctypes.c_void_p, ctypes.c_int
    assert L.GradAccumArgs._fields_ == [("slots", p), ("blocks", p), ("nslots", i), ("nblocks", i), ("acc", p), ("inv_k", ctypes.c_float), ("op", i)]
    assert [f for f, _ in L.GradAccumArgs._fields_[:4]] == [f for f, _ in L.EmaArgs._fields_[:4]], "the table fields every table kernel starts with"
    assert (L.SRK_ACCUM_ADD, L.SRK_ACCUM_FINAL) == (0, 1)

    def refused(msg, **kw):
        base = dict(slots=16, blocks=16, nslots=1, nblocks=2, acc=16, inv_k=0.5, op=L.SRK_ACCUM_ADD)      # (never dereferenced)
        base.update(kw)
        assert lib.srk_grad_accum(ctypes.byref(L.GradAccumArgs(**base)), None) == L.SRK_E_BADARG, kw
        assert msg in lib.srk_last_error(), (kw, lib.srk_last_error())
    refused(b"null", slots=None)
    refused(b"null", blocks=None)
    refused(b"null", acc=None)
    refused(b"0 blocks", nblocks=0)
    refused(b"0 tensors", nslots=0)
    refused(b"op 2", op=2)
    refused(b"op -1", op=-1)
    refused(b"inv_k", inv_k=0.0)
    refused(b"inv_k", inv_k=1.5)
    refused(b"inv_k", inv_k=float("nan"))


def test_documented_numbers_follow_from_the_profile_file():
    """INTEGRATION.md's "Gradient accumulation" table is generated from profiles/grad_accum.txt (tools/gen_results.py grad_accum)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_results.py"), "grad_accum", "--check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("<!-- results:grad_accum:begin -->"):text.index("<!-- results:grad_accum:end -->")]
    assert "edsr_large" in table and "edsr_baseline" in table and table.count("\n|") >= 4
