"""GPU test of the walk every table kernel of csrc/optim.hip shares (csrc/param_table.h): the 16-byte path and the scalar path give
the same bits.

Two twin parameter sets hold identical values.  In twin A every parameter and every gradient owns its storage (16-byte aligned: the
4 x float4 path with its scalar tail); in twin B each is `base[1:]` of a storage one element larger (4-byte aligned only: the scalar
path).  Sizes 1 ... 8193 cover a lone tail, exact multiples of 4 and of the 4096-element block, and two and three blocks.  After four
steps with fresh gradients -- Ranger(k=2) has its first step and two Lookahead syncs in them, SGD its first-step momentum buffer --
the twins are `torch.equal` in every parameter and every state tensor, with and without a `DeviceGradScaler`, and twin A is within
the bound the optimizer's own test file sets against its float64 restatement (Adam: torch.optim.Adam on float64 CPU copies, with
test_gpu_optim.py's bounds)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ranger_ref import RangerRef  # noqa: E402
from test_gpu_ranger import _check_against as _check_ranger, _np  # noqa: E402
from test_gpu_sgd_rmsprop import _check_against as _check_torch64, _oracle, _set64  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8193]
STEPS = 4
CASES = {"Adam": dict(), "Ranger": dict(k=2), "SGD": dict(momentum=0.9, dampening=0.1, weight_decay=1e-2),
         "RMSprop": dict(momentum=0.9, centered=True)}


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


def _values(seed, scale_by_index):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) - 0.5) * (10.0 ** (i % 4 - 2) if scale_by_index else 1.0) for i, n in enumerate(SIZES)]


def _place(x, aligned):
    """`x` on the GPU: in a storage of its own, or as base[1:] of one that is an element larger."""
    if aligned:
        t = x.cuda()
    else:
        t = torch.empty(x.numel() + 1, device="cuda")[1:]
        t.copy_(x)
    assert t.is_contiguous() and (t.data_ptr() % 16 == 0) == aligned and t.data_ptr() % 4 == 0
    return t


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Four steps of the float64 restatement on the twins' values and gradients: (reference, its float64 parameters or None)."""
    kw = CASES[name]
    start = _values(1, False)
    if name == "Ranger":
        ref, qs = RangerRef([x.double().numpy() for x in start], **kw), None
    else:
        qs, ref = _oracle(name, start, kw)
    for step in range(STEPS):
        gs = _values(1000 + step, True)
        if name == "Ranger":
            ref.step(_np(gs))
        else:
            _set64(qs, gs)
            ref.step()
    return ref, qs


def _check_adam(opt, ps, ref, qs):
    for p, q in zip(ps, qs):
        st, rst = opt.state[p], ref.state[q]
        err = {"p": float((p.detach().double().cpu() - q.detach()).abs().max())}
        for key in ("exp_avg", "exp_avg_sq"):
            err[key] = float((st[key].double().cpu() - rst[key]).abs().max())
        print("Adam n=%d: max |err| %s" % (p.numel(), err))
        assert err["p"] <= 2e-6 * max(1.0, float(q.detach().abs().max())), p.shape
        assert err["exp_avg"] <= 1e-5 * float(rst["exp_avg"].abs().max()) + 1e-12, p.shape
        assert err["exp_avg_sq"] <= 1e-5 * float(rst["exp_avg_sq"].abs().max()) + 1e-20, p.shape
        assert float(st["step"]) == float(rst["step"])


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "grad_scaler"])
@pytest.mark.parametrize("name", list(CASES))
def test_vector_and_scalar_paths_agree_bit_for_bit(A, name, scaled):
    twins = []
    for aligned in (True, False):
        ps = [torch.nn.Parameter(_place(x, aligned)) for x in _values(1, False)]
        opt = getattr(A.optim, name)(ps, **CASES[name])
        sc = A.optim.DeviceGradScaler("cuda") if scaled else None
        for step in range(STEPS):
            scale = sc.get_scale() if scaled else 1.0        # a power of two: g * scale / scale is g
            for p, g in zip(ps, _values(1000 + step, True)):
                p.grad = _place(g * scale, aligned)
            opt.step(grad_scaler=sc)
        torch.cuda.synchronize()
        assert sc is None or sc.skipped_steps == 0
        twins.append((ps, opt))
    (pa, oa), (pb, ob) = twins
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach()), ("p", a.numel())
        assert set(oa.state[a]) == set(ob.state[b])
        for key, val in oa.state[a].items():
            assert torch.equal(val, ob.state[b][key]), (key, a.numel())
    ref, qs = _reference(name)
    if name == "Ranger":
        _check_ranger(oa, pa, ref, name)
    elif name == "Adam":
        _check_adam(oa, pa, ref, qs)
    else:
        _check_torch64(oa, pa, ref, qs, name)
