"""CPU tests of sr_amd.optim.SGD / sr_amd.optim.RMSprop (the reference's `optimizer: SGD` / `RMSprop`): the ctypes structs
against the header, the model's optimizer table, CPU parameters stepping through the torch classes bit for bit, state dicts
that go to torch.optim and back, and what the constructors reject."""
import copy
import ctypes

import pytest
import torch

import sr_amd


SHAPES = [(1,), (3,), (7, 5, 3, 3), (4097,), (33, 10)]
SGD_HYPER = [dict(), dict(lr=3e-2, momentum=0.9), dict(lr=3e-2, momentum=0.9, dampening=0.1, weight_decay=1e-2),
             dict(lr=3e-2, momentum=0.9, nesterov=True, weight_decay=1e-2, maximize=True)]
RMS_HYPER = [dict(), dict(lr=1e-3, alpha=0.9, weight_decay=1e-2), dict(momentum=0.9), dict(centered=True),
             dict(lr=3e-3, alpha=0.95, eps=1e-6, momentum=0.5, centered=True, weight_decay=1e-2, maximize=True)]
CASES = [("SGD", kw) for kw in SGD_HYPER] + [("RMSprop", kw) for kw in RMS_HYPER]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.rand(*s, generator=g) - 0.5) for s in SHAPES]


def _grads(step, skip=()):
    g = torch.Generator().manual_seed(1000 + step)
    return [None if i in skip else (torch.rand(*s, generator=g) - 0.5) * 10.0 ** (i % 3 - 1) for i, s in enumerate(SHAPES)]


def _skip(step):
    return {0: (1,), 1: (1,), 2: (1, 3), 5: (2,)}.get(step, ())     # tensor 1's first gradient arrives at step 3


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.clone()


@pytest.mark.parametrize("name", ["sgd", "rmsprop"])
def test_args_mirror_the_header(name):
    st = {"sgd": sr_amd._lib.SgdArgs, "rmsprop": sr_amd._lib.RmspropArgs}[name]
    assert sr_amd._lib.STRUCTS["srk_%s_args" % name] is st       # its layout: tests/test_host_surface.py
    for sfx in ("_step", "_step_scaled", "_check_scaled", "_update_scaled"):
        assert sr_amd._lib.PROTOTYPES["srk_%s%s" % (name, sfx)][0] is ctypes.c_int, sfx
        assert ("srk_%s%s" % (name, sfx)) in set(sr_amd._lib.LAUNCHERS) | set(sr_amd._lib.OTHER_SYMBOLS)


def test_entry_points_reject_bad_arguments():
    lib = sr_amd._lib.load()
    for fn, st in ((lib.srk_sgd_step, sr_amd._lib.SgdArgs), (lib.srk_rmsprop_step, sr_amd._lib.RmspropArgs)):
        assert fn(ctypes.byref(st()), None) != 0                                  # NULL table
        assert b"null" in lib.srk_last_error()
        a = st(slots=16, blocks=16, nslots=-1, nblocks=-1)                         # (never dereferenced: the counts are checked first)
        assert fn(ctypes.byref(a), None) != 0
        assert b"-1 blocks" in lib.srk_last_error()


def test_srmodel_builds_the_hip_classes_at_torchs_defaults():
    m = sr_amd.SRCNN(optimizer="SGD", optimizer_params=["lr=0.5", "momentum=0.9"])
    opt = m.configure_optimizers()[0]
    assert type(opt) is sr_amd.optim.SGD and isinstance(opt, torch.optim.SGD)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"], g["maximize"]) == (1e-3, 0, 0, 0, False, False)
    m = sr_amd.SRCNN(optimizer="RMSprop", optimizer_params=["lr=0.5", "centered=True"])
    opt = m.configure_optimizers()[0]
    assert type(opt) is sr_amd.optim.RMSprop and isinstance(opt, torch.optim.RMSprop)
    g = opt.param_groups[0]
    assert (g["lr"], g["alpha"], g["eps"], g["weight_decay"], g["momentum"], g["centered"], g["maximize"]) == \
        (1e-2, 0.99, 1e-8, 0, 0, False, False)
    ref = torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(1))])
    assert set(g) == set(ref.param_groups[0])
    assert set(sr_amd.optim.SGD([torch.nn.Parameter(torch.zeros(1))]).param_groups[0]) == \
        set(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))]).param_groups[0])


@pytest.mark.parametrize("name,kw", CASES)
def test_cpu_parameters_step_like_torch_bit_for_bit(name, kw):
    ps, qs = _params(1), _params(1)
    opt, ref = getattr(sr_amd.optim, name)(ps, **kw), getattr(torch.optim, name)(qs, **kw)
    for step in range(8):
        gs = _grads(step, skip=_skip(step))
        _set(ps, gs)
        _set(qs, gs)
        opt.step()
        ref.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q), p.shape
        assert set(opt.state[p]) == set(ref.state[q])
        for key, val in ref.state[q].items():
            assert torch.equal(opt.state[p][key], val), key


@pytest.mark.parametrize("name,kw", CASES)
def test_state_dict_goes_to_torch_and_back(name, kw):
    """4 steps here -> state_dict -> torch.optim continues 2 steps -> its state_dict -> back here for 2 more: the parameters of an
    uninterrupted torch run, bit for bit."""
    hip_cls, torch_cls = getattr(sr_amd.optim, name), getattr(torch.optim, name)
    ps, rs = _params(2), _params(2)
    opt, whole = hip_cls(ps, **kw), torch_cls(rs, **kw)
    for step in range(8):
        _set(rs, _grads(step, skip=_skip(step)))
        whole.step()
    for step in range(4):
        _set(ps, _grads(step, skip=_skip(step)))
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    mid = torch_cls(qs, **kw)
    mid.load_state_dict(sd)
    for step in range(4, 6):
        _set(qs, _grads(step, skip=_skip(step)))
        mid.step()
    ts = [torch.nn.Parameter(q.detach().clone()) for q in qs]
    back = hip_cls(ts, **kw)
    back.load_state_dict(copy.deepcopy(mid.state_dict()))
    for step in range(6, 8):
        _set(ts, _grads(step, skip=_skip(step)))
        back.step()
    for t, r in zip(ts, rs):
        assert torch.equal(t, r), t.shape
    want = {"SGD": {"momentum_buffer"} if kw.get("momentum") else set(),
            "RMSprop": {"step", "square_avg"} | ({"momentum_buffer"} if kw.get("momentum") else set()) | ({"grad_avg"} if kw.get("centered") else set())}[name]
    for st in back.state_dict()["state"].values():
        assert set(st) == want


@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_constructor_rejections(name):
    cls = getattr(sr_amd.optim, name)
    with pytest.raises(NotImplementedError):
        cls(_params(3), differentiable=True)
    with pytest.raises(NotImplementedError):
        cls(_params(3), lr=torch.tensor(1e-3))
    for kw in (dict(lr=-1e-3), dict(weight_decay=-1e-4), dict(momentum=-0.5)):
        with pytest.raises(ValueError):
            cls(_params(3), **kw)
    cls(_params(3), foreach=False)                               # accepted
    if name == "SGD":
        with pytest.raises(NotImplementedError):
            cls(_params(3), fused=True)
        with pytest.raises(ValueError, match="Nesterov"):
            cls(_params(3), nesterov=True)
        with pytest.raises(ValueError, match="Nesterov"):
            cls(_params(3), momentum=0.9, dampening=0.1, nesterov=True)
    else:
        cls(_params(3), capturable=False)
        for kw in (dict(eps=-1e-8), dict(alpha=-0.1)):
            with pytest.raises(ValueError):
                cls(_params(3), **kw)


@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_sparse_gradients_raise(name):
    p = torch.nn.Parameter(torch.zeros(4))
    opt = getattr(sr_amd.optim, name)([p])
    p.grad = torch.zeros(4).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()


def test_graphed_step_watches_the_new_hyper_parameters():
    """A change of dampening / nesterov / centered re-captures the graph (the launch takes them by value), and a restored
    snapshot gives booleans back as booleans."""
    from sr_amd import trainer as T
    p = torch.nn.Parameter(torch.zeros(4))
    for opt, key, new in ((sr_amd.optim.SGD([p], momentum=0.9), "dampening", 0.5), (sr_amd.optim.SGD([p], momentum=0.9), "nesterov", True),
                          (sr_amd.optim.RMSprop([p]), "centered", True)):
        g = T.GraphedStep.__new__(T.GraphedStep)
        g.opt = opt
        before = g._hyper()
        old = opt.param_groups[0][key]
        opt.param_groups[0][key] = new
        assert g._hyper() != before, key
        g._set_hyper(before)
        assert opt.param_groups[0][key] == old, key
        if isinstance(old, bool):
            assert opt.param_groups[0][key] is old, key
        assert g._hyper() == before
