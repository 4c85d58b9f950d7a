"""CPU tests of sr_amd.optim.Ranger (torch_optimizer 0.3.0's Ranger; the reference's `optimizer: Ranger`): its plain-torch
CPU form against the float64 restatement in ranger_ref.py, the state and group layout, the constructor's checks, and the
model's optimizer table."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import sr_amd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ranger_ref import RangerRef, scalars  # noqa: E402


SHAPES = [(1,), (3,), (7, 5, 3, 3), (4097,), (33, 10)]
HYPER = [dict(), dict(lr=3e-2, betas=(0.9, 0.99), alpha=0.8, k=3, weight_decay=1e-2)]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.rand(*s, generator=g) - 0.5) for s in SHAPES]


def _grads(step, skip=()):
    g = torch.Generator().manual_seed(1000 + step)
    return [None if i in skip else (torch.rand(*s, generator=g) - 0.5) * 10.0 ** (i % 3 - 1) for i, s in enumerate(SHAPES)]


@pytest.mark.parametrize("kw", HYPER)
def test_cpu_form_matches_float64_reference(kw):
    ps = _params(1)
    opt = sr_amd.optim.Ranger(ps, **kw)
    ref = RangerRef([p.detach().numpy() for p in ps], **kw)
    for step in range(20):
        gs = _grads(step, skip=(1,) if step in (2, 9) else ())
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
        ref.step([None if g is None else g.numpy() for g in gs])
    for i, p in enumerate(ps):
        r = ref.p[i]
        scale = max(1.0, float(np.abs(r).max()))
        assert float(np.abs(p.detach().numpy() - r).max()) <= 1e-5 * scale, SHAPES[i]
        st = opt.state[p]
        assert st["step"] == ref.step_count[i]
        for key, want in (("exp_avg", ref.m[i]), ("exp_avg_sq", ref.v[i]), ("slow_buffer", ref.slow[i])):
            assert float(np.abs(st[key].numpy() - want).max()) <= 1e-5 * max(float(np.abs(want).max()), 1e-30), key
    assert ref.step_count[1] == 18 and ref.step_count[0] == 20


def test_rectification_starts_at_step_6_with_the_defaults():
    flags = [scalars(t, 0.95, 0.999, 5)[1] for t in range(1, 8)]
    assert flags == [False] * 5 + [True, True]
    assert [sr_amd.optim.ranger_scalars(t, 0.95, 0.999, 5)[0] for t in range(1, 8)] == flags
    for t in (1, 5, 6, 12):
        assert sr_amd.optim.ranger_scalars(t, 0.95, 0.999, 5)[1] == pytest.approx(scalars(t, 0.95, 0.999, 5)[2], rel=1e-14)
    # the optimizer itself: step 5 moves by -s*lr*m, step 6 by -s*lr*m/(sqrt(v)+eps)
    p = torch.nn.Parameter(torch.zeros(8))
    opt = sr_amd.optim.Ranger([p])
    g = torch.linspace(-1.0, 1.0, 8)
    for t in range(1, 7):
        before = p.detach().clone()
        p.grad = g.clone()
        opt.step()
        st = opt.state[p]
        _, rect, s = scalars(t, 0.95, 0.999, 5)
        u = st["exp_avg"] / (st["exp_avg_sq"].sqrt() + 1e-5) if rect else st["exp_avg"]
        want = before - s * 1e-3 * u
        if t == 6:                                       # and the Lookahead sync: slow (= the start, 0) + 0.5 * (fast - slow)
            want = 0.5 * want
        torch.testing.assert_close(p.detach(), want, rtol=1e-5, atol=1e-9)


def test_state_dict_and_group_keys():
    ps = _params(2)
    opt = sr_amd.optim.Ranger(ps)
    for step in range(3):
        for p, g in zip(ps, _grads(step)):
            p.grad = g
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "slow_buffer"}
    assert set(sd["param_groups"][0]) == {"lr", "alpha", "k", "step_counter", "betas", "N_sma_threshhold", "eps", "weight_decay", "params"}
    g = sd["param_groups"][0]
    assert (g["lr"], g["alpha"], g["k"], g["step_counter"], tuple(g["betas"]), g["N_sma_threshhold"], g["eps"], g["weight_decay"]) == \
        (1e-3, 0.5, 6, 0, (0.95, 0.999), 5, 1e-5, 0)
    # a fresh optimizer resumes from it (int steps) and continues like the uninterrupted one
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = sr_amd.optim.Ranger(qs)
    opt2.load_state_dict(sd)
    for step in range(3, 8):
        for p, q, g in zip(ps, qs, _grads(step)):
            p.grad, q.grad = g, g.clone()
        opt.step()
        opt2.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)


@pytest.mark.parametrize("kw", [dict(lr=0.0), dict(lr=-1e-3), dict(alpha=-0.1), dict(alpha=1.5), dict(k=0), dict(betas=(1.0, 0.999)),
                                dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.999)), dict(eps=-1e-8), dict(weight_decay=-1e-4)])
def test_constructor_rejects_bad_hyper_parameters(kw):
    with pytest.raises(ValueError):
        sr_amd.optim.Ranger(_params(3), **kw)


def test_sparse_gradients_raise():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = sr_amd.optim.Ranger([p])
    p.grad = torch.zeros(4).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()


def test_srmodel_builds_ranger_at_the_defaults():
    m = sr_amd.SRCNN(optimizer="Ranger", optimizer_params=["lr=0.5", "k=2"])
    opt = m.configure_optimizers()[0]
    assert isinstance(opt, sr_amd.optim.Ranger)
    g = opt.param_groups[0]
    assert (g["lr"], g["alpha"], g["k"], tuple(g["betas"]), g["N_sma_threshhold"], g["eps"], g["weight_decay"]) == \
        (1e-3, 0.5, 6, (0.95, 0.999), 5, 1e-5, 0)
    for name in ("RangerVA", "RangerQH"):
        with pytest.raises(NotImplementedError):
            sr_amd.SRCNN(optimizer=name)


def test_ranger_args_mirror_the_header():
    assert sr_amd._lib.STRUCTS["srk_ranger_args"] is sr_amd._lib.RangerArgs       # its layout: tests/test_host_surface.py
    assert sr_amd._lib.LAUNCHERS["srk_ranger_step"] is sr_amd._lib.RangerArgs
