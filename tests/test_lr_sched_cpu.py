"""CPU tests of the learning-rate schedules (sr_amd.lr_sched): the float64 closed forms of tests/lr_sched_ref.py against
torch.optim.lr_scheduler driven step by step, `DeviceLRSchedule` on CPU parameters under each of the four optimizers, the state-dict
round trip, what the constructor and the C entry point reject, and the `SRModel` / train.py surface."""
import ctypes
import os
import sys
import warnings

import pytest
import torch
from torch.optim import lr_scheduler as S

import sr_amd
from sr_amd.lr_sched import DeviceLRSchedule

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lr_sched_ref as R  # noqa: E402

BASES = (2e-4, 1e-3)
SHAPES = [(3,), (7, 5, 3, 3), (1025,)]

# (name, torch scheduler factory, the closed form as lr_sched_ref.lr keywords, steps)
TORCH_CASES = [
    ("step", lambda o: S.StepLR(o, 7, 0.5), dict(kind="step", step_size=7, gamma=0.5), 200),
    ("multistep", lambda o: S.MultiStepLR(o, [3, 10, 11, 50], 0.3), dict(kind="multistep", milestones=[3, 10, 11, 50], gamma=0.3), 100),
    ("cosine", lambda o: S.CosineAnnealingLR(o, 100, 1e-7), dict(kind="cosine", t_max=100, eta_min=1e-7), 101),
    ("cosine_past_t_max", lambda o: S.CosineAnnealingLR(o, 20, 1e-7), dict(kind="cosine", t_max=20, eta_min=1e-7), 90),
    ("restarts_5_2", lambda o: S.CosineAnnealingWarmRestarts(o, 5, 2, 1e-7), dict(kind="cosine_restarts", t_0=5, t_mult=2, eta_min=1e-7), 200),
    ("restarts_7_1", lambda o: S.CosineAnnealingWarmRestarts(o, 7, 1, 0), dict(kind="cosine_restarts", t_0=7, t_mult=1, eta_min=0.0), 100),
    ("warm_step", lambda o: S.ChainedScheduler([S.LinearLR(o, 0.1, 1.0, 9), S.StepLR(o, 7, 0.5)]),
     dict(kind="step", step_size=7, gamma=0.5, warmup_steps=9, warmup_start=0.1), 60),
    ("warm_multistep", lambda o: S.ChainedScheduler([S.LinearLR(o, 0.2, 1.0, 4), S.MultiStepLR(o, [3, 10], 0.5)]),
     dict(kind="multistep", milestones=[3, 10], gamma=0.5, warmup_steps=4, warmup_start=0.2), 30),
    ("warm_cosine_eta0", lambda o: S.ChainedScheduler([S.LinearLR(o, 0.01, 1.0, 5), S.CosineAnnealingLR(o, 40, 0.0)]),
     dict(kind="cosine", t_max=40, eta_min=0.0, warmup_steps=5, warmup_start=0.01), 40),
]


@pytest.mark.parametrize("name,make,kw,steps", TORCH_CASES, ids=[c[0] for c in TORCH_CASES])
def test_closed_forms_against_torch(name, make, kw, steps):
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in BASES]
    opt = torch.optim.SGD([{"params": [p], "lr": b} for p, b in zip(ps, BASES)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sch = make(opt)
        worst = 0.0
        for t in range(steps):
            for g, b in zip(opt.param_groups, BASES):
                want, got = float(g["lr"]), R.lr(t=t, base=b, **kw)
                worst = max(worst, abs(got - want) / b)
                assert abs(got - want) <= R.TOL * b, (name, t, b, got, want)
            opt.step()
            sch.step()
    print(f"{name}: worst |closed form - torch| / base = {worst:.3g}")


# ---- DeviceLRSchedule on CPU parameters ------------------------------------------------------------------------------------------
SCHEDULES = [
    ("constant", dict(warmup_steps=4, warmup_start=0.25)),
    ("step", dict(step_size=3, gamma=0.5)),
    ("multistep", dict(milestones=[2, 5, 6], gamma=0.3, warmup_steps=3, warmup_start=0.1)),
    ("cosine", dict(t_max=6, eta_min=1e-7)),
    ("cosine_restarts", dict(t_0=3, t_mult=2, eta_min=1e-7, warmup_steps=2, warmup_start=0.5)),
]
OPTIMIZERS = [("Adam", dict()), ("Ranger", dict(k=3)), ("SGD", dict(momentum=0.9, nesterov=True)), ("RMSprop", dict(centered=True, momentum=0.5))]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.rand(*s, generator=g) - 0.5) for s in SHAPES]


def _grads(step):
    g = torch.Generator().manual_seed(1000 + step)
    return [(torch.rand(*s, generator=g) - 0.5) * 10.0 ** (i % 3 - 1) for i, s in enumerate(SHAPES)]


def _make(name, kw, ps):
    return getattr(sr_amd.optim, name)([{"params": ps[:2], "lr": BASES[0]}, {"params": ps[2:], "lr": BASES[1]}], **kw)


def _state_equal(oa, pa, ob, pb):
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
        assert set(oa.state[a]) == set(ob.state[b])
        for key, v in oa.state[a].items():
            w = ob.state[b][key]
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(w)), key


@pytest.mark.parametrize("kind,consts", SCHEDULES, ids=[s[0] for s in SCHEDULES])
@pytest.mark.parametrize("name,kw", OPTIMIZERS, ids=[o[0] for o in OPTIMIZERS])
def test_cpu_trajectory_is_the_optimizer_with_lr_set_by_hand(name, kw, kind, consts):
    pa, pb = _params(1), _params(1)
    oa, ob = _make(name, kw, pa), _make(name, kw, pb)
    sched = DeviceLRSchedule(oa, kind, **consts)
    assert oa.lr_schedule is sched and not sched.on_gpu
    for t in range(14):
        want = [R.lr(kind, t, b, **consts) for b in BASES]
        assert sched.get_last_lr() == want and [g["lr"] for g in oa.param_groups] == want and sched.device_lr() == want
        for g, v in zip(ob.param_groups, want):
            g["lr"] = v
        for p, q, g in zip(pa, pb, _grads(t)):
            p.grad, q.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    assert sched.count == 14
    _state_equal(oa, pa, ob, pb)


def test_state_dict_round_trip_continues_with_the_same_values():
    consts = dict(t_0=3, t_mult=2, eta_min=1e-7, warmup_steps=2, warmup_start=0.5)
    pa, pb = _params(2), _params(2)
    oa, ob = _make("Adam", {}, pa), _make("Adam", {}, pb)
    sa, sb = DeviceLRSchedule(oa, "cosine_restarts", **consts), DeviceLRSchedule(ob, "cosine_restarts", **consts)
    for t in range(12):
        if t == 5:                           # the second run swaps its schedule for a new one that loads the old one's state
            sd = sb.state_dict()
            assert sd == dict(kind="cosine_restarts", constants=consts, count=5, base_lrs=list(BASES))
            sb.detach()
            sb = DeviceLRSchedule(ob, "constant")             # (its own bases are the detached, decayed values: the state's replace them)
            sb.load_state_dict(sd)
            assert sb.count == 5 and sb.kind == "cosine_restarts" and sb.constants == sa.constants and sb.base_lrs == list(BASES)
            assert [g["lr"] for g in ob.param_groups] == [R.lr("cosine_restarts", 5, b, **consts) for b in BASES]
        for p, q, g in zip(pa, pb, _grads(t)):
            p.grad, q.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    assert sb.count == sa.count == 12
    assert sb.get_last_lr() == sa.get_last_lr() == [R.lr("cosine_restarts", 12, b, **consts) for b in BASES]
    _state_equal(oa, pa, ob, pb)
    with pytest.raises(ValueError, match="parameter groups"):
        sb.load_state_dict(dict(sd, base_lrs=[1e-3]))


def test_detach_returns_the_groups_to_lr_by_value():
    ps = _params(3)
    opt = _make("SGD", {}, ps)
    sched = DeviceLRSchedule(opt, "step", step_size=2, gamma=0.5)
    with pytest.raises(RuntimeError, match="already has"):
        DeviceLRSchedule(opt, "constant")
    for t in range(3):
        for p, g in zip(ps, _grads(t)):
            p.grad = g
        opt.step()
    sched.detach()
    assert opt.lr_schedule is None and [g["lr"] for g in opt.param_groups] == [b * 0.5 for b in BASES]
    opt.step()
    assert [g["lr"] for g in opt.param_groups] == [b * 0.5 for b in BASES], "no hook is left"


def test_manual_schedule_writes_what_set_lr_says():
    ps = _params(4)
    opt = _make("SGD", {}, ps)
    sched = DeviceLRSchedule(opt, "manual")
    assert sched.get_last_lr() == list(BASES)
    sched.set_lr([3e-3, 4e-3])
    assert [g["lr"] for g in opt.param_groups] == [3e-3, 4e-3] == sched.get_last_lr()
    sched.set_lr(5e-4)
    assert [g["lr"] for g in opt.param_groups] == [5e-4, 5e-4]
    with pytest.raises(ValueError):
        sched.set_lr([1e-3])
    other = DeviceLRSchedule(_make("SGD", {}, _params(5)), "constant")
    with pytest.raises(RuntimeError, match="manual"):
        other.set_lr(1e-3)


@pytest.mark.parametrize("kind,consts,match", [
    ("exponential", dict(gamma=0.9), "not recognized"),                        # an unknown kind
    ("step", dict(gamma=0.5), "needs step_size"),                              # a missing constant
    ("cosine", dict(), "needs t_max"),
    ("cosine_restarts", dict(t_mult=2), "needs t_0"),
    ("multistep", dict(gamma=0.5), "needs milestones"),
    ("step", dict(step_size=3, t_max=5), "no constant t_max"),                 # an unknown constant
    ("manual", dict(warmup_steps=3), "no constant warmup_steps"),
    ("multistep", dict(milestones=list(range(17))), "17 milestones"),          # a 17th milestone
    ("multistep", dict(milestones=[5, 3]), "not sorted"),
    ("step", dict(step_size=0), "step_size=0"),
    ("cosine", dict(t_max=0), "t_max=0"),
    ("cosine_restarts", dict(t_0=0), "t_0=0"),
    ("cosine_restarts", dict(t_0=3, t_mult=0), "t_mult=0"),
    ("step", dict(step_size=2, warmup_steps=3, warmup_start=0), "warmup_start"),
    ("step", dict(step_size=2, warmup_steps=3, warmup_start=1.5), "warmup_start"),
    ("step", dict(step_size=2.5), "not an integer"),
])
def test_constructor_rejections(kind, consts, match):
    opt = _make("Adam", {}, _params(6))
    with pytest.raises(ValueError, match=match):
        DeviceLRSchedule(opt, kind, **consts)
    assert opt.lr_schedule is None and not opt._optimizer_step_post_hooks, "nothing stays attached"
    DeviceLRSchedule(opt, "multistep", milestones=list(range(16)))            # sixteen are fine


def test_entry_point_rejects_bad_constants():
    """srk_lr_sched_step checks its arguments before it launches anything (no GPU is touched: every call here is refused)."""
    L = sr_amd._lib
    lib = L.load()
    assert L.LAUNCHERS["srk_lr_sched_step"] is L.LrSchedArgs is L.STRUCTS["srk_lr_sched_args"]
    assert (L.SRK_LR_CONSTANT, L.SRK_LR_STEP, L.SRK_LR_MULTISTEP, L.SRK_LR_COSINE, L.SRK_LR_COSINE_RESTARTS) == (0, 1, 2, 3, 4)
    assert (L.LR_SET, L.LR_ADVANCE) == (L.SRK_LR_SET, L.SRK_LR_ADVANCE) == (0, 1) and L.SRK_LR_MAX_MILESTONES == 16
    for st in (L.AdamArgs, L.RangerArgs, L.SgdArgs, L.RmspropArgs):
        assert st._fields_[-1] == ("lr_dev", ctypes.c_void_p), st.__name__
        assert st().lr_dev is None, "callers that do not name it pass NULL: the by-value path"

    def refused(msg, **kw):
        base = dict(count=16, lr=16, base_lr=16, ngroups=2, warmup_start=1.0)      # (never dereferenced: the checks come first)
        base.update(kw)
        assert lib.srk_lr_sched_step(ctypes.byref(L.LrSchedArgs(**base)), None) == L.SRK_E_BADARG, kw
        assert msg in lib.srk_last_error(), (kw, lib.srk_last_error())
    refused(b"null", count=None)
    refused(b"0 groups", ngroups=0)
    refused(b"kind 5", kind=5)
    refused(b"op 2", op=2)
    refused(b"count -1", op=L.LR_SET, value=-1)
    refused(b"step_size=0", kind=L.SRK_LR_STEP, step_size=0)
    refused(b"t_max=0", kind=L.SRK_LR_COSINE, t_max=0)
    refused(b"t_0=0", kind=L.SRK_LR_COSINE_RESTARTS, t_0=0, t_mult=1)
    refused(b"t_mult=0", kind=L.SRK_LR_COSINE_RESTARTS, t_0=1, t_mult=0)
    refused(b"not sorted", kind=L.SRK_LR_MULTISTEP, nmilestones=3, m0=1, m1=5, m2=4)
    refused(b"17 milestones", kind=L.SRK_LR_MULTISTEP, nmilestones=17)
    refused(b"warmup_start=0", kind=L.SRK_LR_STEP, step_size=1, warmup_steps=2, warmup_start=0.0)
    refused(b"warmup_start=1.5", kind=L.SRK_LR_STEP, step_size=1, warmup_steps=2, warmup_start=1.5)


# ---- the model and train.py -----------------------------------------------------------------------------------------------------------
def test_srmodel_attaches_the_schedule_to_its_optimizer():
    m = sr_amd.SRCNN(scale_factor=2, lr_schedule="cosine", lr_schedule_params=["t_max=300000", "eta_min=1e-7", "warmup_steps=2000", "warmup_start=0.01"])
    opts = m.configure_optimizers()
    assert len(opts) == 1 and isinstance(opts[0], sr_amd.optim.Adam)
    sched = opts[0].lr_schedule
    assert isinstance(sched, DeviceLRSchedule) and sched.kind == "cosine"
    assert sched.constants == dict(t_max=300000, eta_min=1e-7, warmup_steps=2000, warmup_start=0.01)
    assert sched.base_lrs == [1e-3] and opts[0].param_groups[0]["lr"] == R.lr("cosine", 0, 1e-3, **sched.constants)
    m2 = sr_amd.SRCNN(scale_factor=2, lr_schedule="multistep", lr_schedule_params=["milestones=200000,400000", "gamma=0.5"])
    assert m2.configure_optimizers()[0].lr_schedule.constants["milestones"] == [200000, 400000]
    # a restored state continues at its count
    m2.lr_schedule_state = dict(kind="multistep", constants=dict(milestones=[2, 4], gamma=0.5), count=3, base_lrs=[1e-3])
    s2 = m2.configure_optimizers()[0].lr_schedule
    assert s2.count == 3 and s2.get_last_lr() == [5e-4]


def test_srmodel_without_a_schedule_builds_nothing():
    m = sr_amd.SRCNN(scale_factor=2)
    opt = m.configure_optimizers()[0]
    assert opt.lr_schedule is None and opt._lr_dev is None and not opt._optimizer_step_post_hooks
    assert sr_amd.SRCNN(scale_factor=2, lr_schedule="").configure_optimizers()[0].lr_schedule is None


@pytest.mark.parametrize("kind,params", [
    ("exponential", []),                                   # an unknown kind
    ("cosine", []),                                        # a missing constant
    ("cosine", ["t_max=10", "gamma=0.5"]),                 # an unknown constant
    ("cosine", ["t_max"]),                                 # not name=value
    ("cosine", ["t_max=ten"]),
    ("step", ["step_size=2.5"]),
    ("multistep", ["milestones=3;4"]),
    ("", ["t_max=10"]),                                    # constants without a schedule
])
def test_srmodel_rejects_bad_schedule_strings(kind, params):
    with pytest.raises(ValueError):
        sr_amd.SRCNN(scale_factor=2, lr_schedule=kind, lr_schedule_params=params)


def test_train_py_saves_and_restores_the_schedule(tmp_path):
    """The CPU plumbing case: two steps with a schedule, --save, then two more from the checkpoint: the count goes on from 2."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(root, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    common = ["-m", "srcnn", "--accelerator", "cpu", "--max_steps", "2", "--batch_size", "2", "--patch_size", "16", "-s", "2", "--precision", "32",
              "--log_every", "0", "--lr_schedule", "step", "--lr_schedule_params", "step_size=1", "gamma=0.5"]
    first, second = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    train.main(common + ["--save", first])
    sd = torch.load(first, map_location="cpu")
    assert sd["lr_schedule"] == dict(kind="step", constants=dict(step_size=1, gamma=0.5, warmup_steps=0, warmup_start=1.0), count=2, base_lrs=[1e-3])
    train.main(common + ["--checkpoint", first, "--save", second])
    assert torch.load(second, map_location="cpu")["lr_schedule"]["count"] == 4
