"""GPU tests of sr_amd.optim.Ranger (csrc/optim.hip: torch_optimizer 0.3.0's Ranger -- RAdam + Lookahead -- over every parameter
tensor in one launch) against the float64 restatement in ranger_ref.py: the trajectory and the state, the double-precision
RAdam scalars, the Lookahead sync, per-tensor step counts, hipGraph replay across the rectification and sync steps, the
device-resident loss scaler, state_dict round trips and Trainer.fit."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ranger_ref import RangerRef  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (64,), (7, 5, 3, 3), (64, 64, 3, 3), (4097,), (33, 1000)]
HYPER = [dict(), dict(lr=3e-2, betas=(0.9, 0.99), alpha=0.8, k=3, weight_decay=1e-2)]


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


def _params(seed, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.rand(*s, generator=g) - 0.5).cuda()) for s in shapes]


def _grads(step, shapes=SHAPES, skip=()):
    """CPU gradients of one step (None for the skipped indices)."""
    g = torch.Generator().manual_seed(1000 + step)
    out = []
    for i, s in enumerate(shapes):
        gr = (torch.rand(*s, generator=g) - 0.5) * (10.0 ** (i % 4 - 2))
        out.append(None if i in skip else gr)
    return out


def _set(ps, gs, scale=1.0):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else (g * scale).cuda()


def _np(gs):
    return [None if g is None else g.double().numpy() for g in gs]


def _close(got, want, what):
    got = got.detach().double().cpu().numpy()
    err = float(np.abs(got - want).max())
    assert err <= 2e-6 * max(1.0, float(np.abs(want).max())), (what, err)


def _check_against(opt, ps, ref, what=""):
    for i, p in enumerate(ps):
        st = opt.state[p]
        _close(p, ref.p[i], (what, "p", p.shape))
        _close(st["exp_avg"], ref.m[i], (what, "exp_avg", p.shape))
        _close(st["exp_avg_sq"], ref.v[i], (what, "exp_avg_sq", p.shape))
        _close(st["slow_buffer"], ref.slow[i], (what, "slow_buffer", p.shape))
        assert float(st["step"]) == ref.step_count[i], (what, p.shape)


def _skip(step):
    # parameters without a gradient on some steps: their counts and Lookahead phases drift from the others'
    return {1: (2,), 4: (2, 5), 7: (3,), 8: (3,), 9: (3,)}.get(step, ())


@pytest.mark.parametrize("kw", HYPER)
def test_matches_float64_reference(A, kw):
    ps = _params(1)
    opt = A.optim.Ranger(ps, **kw)
    assert isinstance(opt, torch.optim.Optimizer)
    ref = RangerRef([p.detach().double().cpu().numpy() for p in ps], **kw)
    for step in range(20):
        gs = _grads(step, skip=_skip(step))
        _set(ps, gs)
        opt.step()
        ref.step(_np(gs))
    torch.cuda.synchronize()
    _check_against(opt, ps, ref)
    assert [float(opt.state[p]["step"]) for p in ps] == [20, 20, 18, 17, 20, 19, 20]


def test_scalars_in_double_and_lookahead_sync(A):
    """From p = 0 at lr = 1e-3 the per-step update follows the float64 rule to fp32 rounding (~1e-4): an fp32 RAdam step size
    would be ~6e-3 off at step 6 (N_sma = 1999 - 1993.0 cancels).  After the sync steps 6 and 12, p IS the slow buffer."""
    shapes = [(4099,), (64, 3, 3, 3)]
    ps = [torch.nn.Parameter(torch.zeros(*s, device="cuda")) for s in shapes]
    opt = A.optim.Ranger(ps, lr=1e-3)
    ref = RangerRef([np.zeros(s) for s in shapes], lr=1e-3)
    for t in range(1, 13):
        gs = _grads(t, shapes)
        before = [p.detach().double().cpu().numpy() for p in ps]
        rbefore = [x.copy() for x in ref.p]
        _set(ps, gs)
        opt.step()
        ref.step(_np(gs))
        if t in (6, 7, 8, 12):
            for p, b, r, rb in zip(ps, before, ref.p, rbefore):
                du, rdu = p.detach().double().cpu().numpy() - b, r - rb
                rel = float(np.linalg.norm(du - rdu) / np.linalg.norm(rdu))
                assert rel <= 1e-3, (t, p.shape, rel)
        if t in (6, 12):
            for p in ps:
                assert torch.equal(p.detach(), opt.state[p]["slow_buffer"]), t
    torch.cuda.synchronize()
    _check_against(opt, ps, ref)


def test_graph_replay_is_bit_identical_to_eager(A):
    """Two eager steps, then opt.step() captured and replayed up to step 14: the replays cross step 6 (rectification starts) and
    the Lookahead syncs at 6 and 12 -- decided on the device from the step counts -- and match an eager run bit for bit."""
    runs = []
    for graphed in (False, True):
        ps = _params(3)
        opt = A.optim.Ranger(ps)
        static = [torch.zeros_like(p) for p in ps]
        for p, s in zip(ps, static):
            p.grad = s
        graph = None
        for step in range(14):
            for s, g in zip(static, _grads(step)):
                s.copy_(g)
            if not graphed or step < 2:
                opt.step()
                continue
            if graph is None:
                opt.reserve_capture_tables()
                graph = torch.cuda.CUDAGraph()
                st = torch.cuda.Stream()
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    with torch.cuda.graph(graph, stream=st):
                        opt.step()
                torch.cuda.current_stream().wait_stream(st)
            graph.replay()
        torch.cuda.synchronize()
        runs.append((ps, opt))
        if graph is not None:
            del graph
            opt.release_captured_tables()
    (pe, oe), (pg, og) = runs
    for a, b in zip(pe, pg):
        assert torch.equal(a.detach(), b.detach()), a.shape
        for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            assert torch.equal(oe.state[a][key], og.state[b][key]), (key, a.shape)
        assert float(og.state[b]["step"]) == 14.0


@pytest.mark.parametrize("groups", [1, 2])
def test_device_grad_scaler_skips_the_step_with_an_inf(A, groups):
    """An inf at step 6 (one group, and in the LAST of two groups): nothing moves -- parameters, moments, slow buffers, step
    counts -- and the scale halves; the later steps follow a reference that never saw that step."""
    shapes = [SHAPES[:4], SHAPES[4:]] if groups == 2 else [SHAPES]
    hyper = [dict(lr=1e-2), dict(lr=3e-3, betas=(0.9, 0.99), k=3)][:groups]
    pss = [_params(7 + i, s) for i, s in enumerate(shapes)]
    opt = A.optim.Ranger([dict(params=ps, **h) for ps, h in zip(pss, hyper)]) if groups == 2 else A.optim.Ranger(pss[0], **hyper[0])
    refs = [RangerRef([p.detach().double().cpu().numpy() for p in ps], **h) for ps, h in zip(pss, hyper)]
    sc = A.optim.DeviceGradScaler("cuda", init_scale=256.0, growth_interval=100)
    allp = [p for ps in pss for p in ps]
    for step in range(1, 15):
        scale = sc.get_scale()
        gss = [_grads(step * 10 + i, s) for i, s in enumerate(shapes)]
        for ps, gs in zip(pss, gss):
            _set(ps, gs, scale)
        if step == 6:
            pss[-1][-1].grad.view(-1)[5] = float("inf")
            before = {id(p): [p.detach().clone()] + [opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq", "slow_buffer", "step")]
                      for p in allp}
        opt.step(grad_scaler=sc)
        if step == 6:
            torch.cuda.synchronize()
            for p in allp:
                now = [p.detach()] + [opt.state[p][k] for k in ("exp_avg", "exp_avg_sq", "slow_buffer", "step")]
                assert all(torch.equal(a, b) for a, b in zip(before[id(p)], now)), p.shape
            assert sc.get_scale() == scale / 2 and sc.skipped_steps == 1
            continue
        for ref, gs in zip(refs, gss):
            ref.step(_np(gs))
    torch.cuda.synchronize()
    for ps, ref in zip(pss, refs):
        _check_against(opt, ps, ref)
    assert float(opt.state[allp[0]]["step"]) == 13.0


@pytest.mark.parametrize("form", ["as_saved", "int_steps_cpu_tensors"])
def test_state_dict_round_trip(A, form):
    kw = HYPER[1]
    ps = _params(5)
    opt = A.optim.Ranger(ps, **kw)
    for step in range(14):
        if step == 4:
            sd = copy.deepcopy(opt.state_dict())
            at4 = [p.detach().clone() for p in ps]
        _set(ps, _grads(step, skip=_skip(step)))
        opt.step()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "slow_buffer"}
    if form == "int_steps_cpu_tensors":
        for st in sd["state"].values():
            for key in list(st):
                st[key] = int(st[key]) if key == "step" else st[key].cpu()
    qs = [torch.nn.Parameter(x) for x in at4]
    opt2 = A.optim.Ranger(qs, **kw)
    opt2.load_state_dict(sd)
    for step in range(4, 14):
        _set(qs, _grads(step, skip=_skip(step)))
        opt2.step()
    torch.cuda.synchronize()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach()), p.shape
        for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            assert torch.equal(opt.state[p][key], opt2.state[q][key]), key
        assert float(opt.state[p]["step"]) == float(opt2.state[q]["step"])


@pytest.mark.parametrize("precision", [32, 16])
def test_trainer_fit_with_ranger_graph_on_and_off(A, precision):
    """EDSR with optimizer="Ranger" through Trainer.fit, 10 steps, graph on and off: the same parameters.  fp16 trains under the
    device-resident loss scaler and still replays a graph."""
    from sr_amd import trainer as T
    out = []
    for use_graph in (True, False):
        torch.manual_seed(0)
        m = A.EDSR(scale_factor=2, precision=precision, n_feats=16, n_resblocks=2, res_scale=0.1, optimizer="Ranger")
        tr = T.Trainer(device="cuda", use_graph=use_graph)
        tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 700 + i, "cpu") for i in range(10)))
        torch.cuda.synchronize()
        if use_graph:
            assert isinstance(tr.graphed.opt, A.optim.Ranger)
        if precision == 16:
            assert tr.scaler is not None and hasattr(tr.scaler, "state") and tr.scaler.skipped_steps == 0
        out.append((tr.losses, [p.detach().clone() for p in m.parameters()], tr.graphed))
    (lg, pg, g), (le, pe, _) = out
    assert g is not None and g.graphs is not None and not g.failed, "the step was captured"
    assert len(lg) == len(le) == 10 and all(np.isfinite(lg))
    np.testing.assert_allclose(lg, le, rtol=2e-4 if precision == 32 else 2e-3)
    for a, b in zip(pg, pe):
        if precision == 32:
            assert float((a - b).abs().max()) <= 2e-4, float((a - b).abs().max())
        else:
            assert float((a - b).abs().max()) <= 9.5e-3 and float((a - b).abs().mean()) <= 3e-4
