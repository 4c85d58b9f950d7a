"""GPU tests of sr_amd.optim.SGD / sr_amd.optim.RMSprop (csrc/optim.hip: torch.optim.SGD / RMSprop over every parameter tensor in
one launch) against the torch classes themselves, run in float64 on CPU copies: the trajectory and every state tensor, SGD's
first-step rule decided on the device, hipGraph replay, the device-resident loss scaler, state dicts that come from and go to
torch.optim, and Trainer.fit.  Parameters and gradients are generated as in test_gpu_ranger.py."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (64,), (7, 5, 3, 3), (64, 64, 3, 3), (4097,), (33, 1000)]
SGD_HYPER = [dict(), dict(lr=3e-2, momentum=0.9), dict(lr=3e-2, momentum=0.9, dampening=0.1, weight_decay=1e-2),
             dict(lr=3e-2, momentum=0.9, nesterov=True, weight_decay=1e-2, maximize=True)]
RMS_HYPER = [dict(), dict(lr=1e-3, alpha=0.9, weight_decay=1e-2), dict(momentum=0.9), dict(centered=True),
             dict(lr=3e-3, alpha=0.95, eps=1e-6, momentum=0.5, centered=True, weight_decay=1e-2, maximize=True)]
CASES = [("SGD", kw) for kw in SGD_HYPER] + [("RMSprop", kw) for kw in RMS_HYPER]
# the configurations with every buffer in use, for the replay / scaler / state-dict tests
FULL = [("SGD", SGD_HYPER[2]), ("RMSprop", RMS_HYPER[4])]


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


def _set64(qs, gs):
    for q, g in zip(qs, gs):
        q.grad = None if g is None else g.double()


def _skip(step):
    # parameters without a gradient on some steps: their counts drift from the others'
    return {1: (2,), 4: (2, 5), 7: (3,), 8: (3,), 9: (3,)}.get(step, ())


def _oracle(name, ps, kw):
    """The torch class on float64 CPU copies of the parameters."""
    qs = [torch.nn.Parameter(p.detach().double().cpu()) for p in ps]
    return qs, getattr(torch.optim, name)(qs, **kw)


def _close(got, want, what):
    got = got.detach().double().cpu().numpy()
    want = want.detach().double().cpu().numpy()
    err = float(np.abs(got - want).max())
    bound = 2e-6 * max(1.0, float(np.abs(want).max()))
    print("%s: max |err| %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, (what, err)


def _check_against(opt, ps, ref, qs, what=""):
    """Parameters and every state tensor the oracle holds; RMSprop's `step` equal."""
    for i, (p, q) in enumerate(zip(ps, qs)):
        _close(p, q, (what, i, "p"))
        want = ref.state.get(q, {})
        got = opt.state.get(p, {})
        for key, val in want.items():
            if key == "step":
                assert float(got["step"]) == float(val), (what, i, "step")
            elif torch.is_tensor(val):
                _close(got[key], val, (what, i, key))
        assert set(got) >= set(want), (what, i)


@pytest.mark.parametrize("name,kw", CASES)
def test_matches_torch_in_float64(A, name, kw):
    ps = _params(1)
    opt = getattr(A.optim, name)(ps, **kw)
    assert isinstance(opt, getattr(torch.optim, name))
    qs, ref = _oracle(name, ps, kw)
    for step in range(20):
        gs = _grads(step, skip=_skip(step))
        _set(ps, gs)
        _set64(qs, gs)
        opt.step()
        ref.step()
    torch.cuda.synchronize()
    _check_against(opt, ps, ref, qs, name)
    want_keys = {"SGD": {"momentum_buffer"} if kw.get("momentum") else set(),
                 "RMSprop": {"step", "square_avg"} | ({"momentum_buffer"} if kw.get("momentum") else set()) | ({"grad_avg"} if kw.get("centered") else set())}[name]
    for p, q in zip(ps, qs):
        assert set(opt.state.get(p, {})) == want_keys == set(ref.state.get(q, {}))
    assert set(opt.state_dict()["state"]) == set(ref.state_dict()["state"])
    if name == "RMSprop":
        assert [float(opt.state[p]["step"]) for p in ps] == [20, 20, 18, 17, 20, 19, 20]


@pytest.mark.parametrize("graphed", [False, True])
def test_sgd_first_step_copies_the_gradient(A, graphed):
    """Tensors 0 and 4 (one block; nine blocks) receive their first gradient at step 5: torch makes momentum_buffer a copy of it,
    whatever `dampening` is (0.5 here: the other branch would give half of it).  Replayed: the graph is captured at step 5, so the
    first step of the two is a replay, and it reads "first" from the device counts."""
    kw = dict(lr=3e-2, momentum=0.9, dampening=0.5)
    late = (0, 4)
    ps = _params(11)
    opt = A.optim.SGD(ps, **kw)
    qs, ref = _oracle("SGD", ps, kw)
    static = [torch.zeros_like(p) for p in ps]
    graph = None
    for step in range(9):
        gs = _grads(step, skip=late if step < 5 else ())
        for p, s, g in zip(ps, static, gs):
            if g is not None:
                s.copy_(g)
                p.grad = s
        _set64(qs, gs)
        ref.step()
        if not graphed or step < 5:
            opt.step()
        else:
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
        if step == 5:
            torch.cuda.synchronize()
            for i in late:
                assert torch.equal(opt.state[ps[i]]["momentum_buffer"], gs[i].cuda()), i
    torch.cuda.synchronize()
    _check_against(opt, ps, ref, qs, "first step")
    if graph is not None:
        del graph
        opt.release_captured_tables()


def test_sgd_momentum_switched_on_later(A):
    """`momentum` set on the group after three plain steps: the buffers appear then, every tensor is "first" at that step (torch has
    no momentum_buffer yet), and the run follows torch's under the same change."""
    kw = dict(lr=3e-2, dampening=0.5)
    ps = _params(13)
    opt = A.optim.SGD(ps, **kw)
    qs, ref = _oracle("SGD", ps, kw)
    for step in range(8):
        if step == 3:
            assert not opt.state_dict()["state"]
            opt.param_groups[0]["momentum"] = ref.param_groups[0]["momentum"] = 0.9
        gs = _grads(step, skip=_skip(step))
        _set(ps, gs)
        _set64(qs, gs)
        opt.step()
        ref.step()
        if step == 3:
            torch.cuda.synchronize()
            assert torch.equal(opt.state[ps[4]]["momentum_buffer"], gs[4].cuda())
    torch.cuda.synchronize()
    _check_against(opt, ps, ref, qs, "momentum from step 3")


@pytest.mark.parametrize("name,kw", FULL)
def test_graph_replay_is_bit_identical_to_eager(A, name, kw):
    """Two eager steps, then opt.step() captured and replayed up to step 14.  Tensor 3 has no gradient during the eager steps: its
    static gradient is attached right before the capture, so its first step is a replay."""
    runs = []
    for graphed in (False, True):
        ps = _params(3)
        opt = getattr(A.optim, name)(ps, **kw)
        static = [torch.zeros_like(p) for p in ps]
        graph = None
        for step in range(14):
            for i, (p, s, g) in enumerate(zip(ps, static, _grads(step))):
                s.copy_(g)
                p.grad = None if (i == 3 and step < 2) else s
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
    for i, (a, b) in enumerate(zip(pe, pg)):
        assert torch.equal(a.detach(), b.detach()), a.shape
        assert set(oe.state[a]) == set(og.state[b])
        for key in oe.state[a]:
            assert torch.equal(oe.state[a][key], og.state[b][key]), (key, a.shape)
        if name == "RMSprop":
            assert float(og.state[b]["step"]) == (12.0 if i == 3 else 14.0)
    # and the run is the oracle's
    qs, ref = _oracle(name, _params(3), kw)
    for step in range(14):
        _set64(qs, _grads(step, skip=(3,) if step < 2 else ()))
        ref.step()
    _check_against(og, pg, ref, qs, "replayed")


def _counts(opt):
    return [opt._plans[gi].steps.clone() for gi in sorted(opt._plans)]


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_device_grad_scaler_skips_the_step_with_an_inf(A, name, groups):
    """An inf at step 6 (one group, and in the LAST tensor of the LAST of two groups): nothing moves -- parameters, buffers, step
    counts, SGD's "first" counts -- and the scale halves; the later steps follow an oracle that never saw that step.  Tensor 1 of
    the first group would have had its first step at 6: it is still "first" at 7."""
    shapes = [SHAPES[:4], SHAPES[4:]] if groups == 2 else [SHAPES]
    hyper = {"SGD": [dict(lr=1e-2, momentum=0.9, dampening=0.5), dict(lr=3e-3, momentum=0.8, nesterov=True, weight_decay=1e-2)],
             "RMSprop": [dict(lr=1e-3, momentum=0.9), dict(lr=3e-3, alpha=0.9, centered=True)]}[name][:groups]
    cls, tcls = getattr(A.optim, name), getattr(torch.optim, name)
    pss = [_params(7 + i, s) for i, s in enumerate(shapes)]
    opt = cls([dict(params=ps, **h) for ps, h in zip(pss, hyper)]) if groups == 2 else cls(pss[0], **hyper[0])
    qss = [[torch.nn.Parameter(p.detach().double().cpu()) for p in ps] for ps in pss]
    ref = tcls([dict(params=qs, **h) for qs, h in zip(qss, hyper)]) if groups == 2 else tcls(qss[0], **hyper[0])
    sc = A.optim.DeviceGradScaler("cuda", init_scale=256.0, growth_interval=100)
    allp = [p for ps in pss for p in ps]
    for step in range(1, 15):
        scale = sc.get_scale()
        gss = [_grads(step * 10 + i, s, skip=(1,) if (i == 0 and step < 6) else ()) for i, s in enumerate(shapes)]
        for ps, gs in zip(pss, gss):
            _set(ps, gs, scale)
        if step == 6:
            pss[-1][-1].grad.view(-1)[5] = float("inf")
            before = {id(p): [p.detach().clone()] + [v.clone() for _, v in sorted(opt.state[p].items())] for p in allp}
            counts = _counts(opt)
        opt.step(grad_scaler=sc)
        if step == 6:
            torch.cuda.synchronize()
            for p in allp:
                now = [p.detach()] + [v for _, v in sorted(opt.state[p].items())]
                assert len(now) == len(before[id(p)]) and all(torch.equal(a, b) for a, b in zip(before[id(p)], now)), p.shape
            assert all(torch.equal(a, b) for a, b in zip(counts, _counts(opt)))
            assert float(_counts(opt)[0][1]) == 0.0
            assert sc.get_scale() == scale / 2 and sc.skipped_steps == 1
            continue
        for qs, gs in zip(qss, gss):
            _set64(qs, gs)
        ref.step()
    torch.cuda.synchronize()
    _check_against(opt, allp, ref, [q for qs in qss for q in qs], (name, groups))
    assert sc.skipped_steps == 1
    if name == "RMSprop":
        assert float(opt.state[allp[0]]["step"]) == 13.0 and float(opt.state[allp[1]]["step"]) == 8.0


def _skip2(step):
    return _skip(step) + ((6,) if step < 6 else ())           # tensor 6's first gradient arrives at step 6, after the save


@pytest.mark.parametrize("form", ["as_saved", "int_steps_cpu_tensors", "through_torch_on_the_cpu"])
@pytest.mark.parametrize("name,kw", FULL)
def test_state_dict_round_trip(A, name, kw, form):
    """Saved at step 4 (tensor 6 has not had a step yet) and loaded into a fresh optimizer -- as saved; as CPU tensors with integer
    steps; as the state dict torch.optim.<name> itself produces on the CPU after loading ours -- the run continues to the bits of
    the uninterrupted one."""
    cls, tcls = getattr(A.optim, name), getattr(torch.optim, name)
    ps = _params(5)
    opt = cls(ps, **kw)
    for step in range(14):
        if step == 4:
            sd = copy.deepcopy(opt.state_dict())
            at4 = [p.detach().clone() for p in ps]
        _set(ps, _grads(step, skip=_skip2(step)))
        opt.step()
    if name == "SGD":
        assert [k for k, st in sd["state"].items() if st["momentum_buffer"] is None] == [6]
        assert all(set(st) == {"momentum_buffer"} for st in sd["state"].values())
    else:
        assert all(set(st) == {"step", "square_avg", "momentum_buffer", "grad_avg"} for st in sd["state"].values())
        assert float(sd["state"][6]["step"]) == 0.0 and float(sd["state"][0]["step"]) == 4.0
    if form == "int_steps_cpu_tensors":
        for st in sd["state"].values():
            for key in list(st):
                st[key] = int(st[key]) if key == "step" else st[key].cpu() if torch.is_tensor(st[key]) else st[key]
    elif form == "through_torch_on_the_cpu":
        on_cpu = tcls([torch.nn.Parameter(x.cpu()) for x in at4], **kw)
        on_cpu.load_state_dict(sd)
        sd = copy.deepcopy(on_cpu.state_dict())
        assert all(not v.is_cuda for st in sd["state"].values() for k, v in st.items() if torch.is_tensor(v) and k != "step")
    qs = [torch.nn.Parameter(x) for x in at4]
    opt2 = cls(qs, **kw)
    opt2.load_state_dict(sd)
    for step in range(4, 14):
        _set(qs, _grads(step, skip=_skip2(step)))
        opt2.step()
    torch.cuda.synchronize()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach()), p.shape
        assert set(opt.state[p]) == set(opt2.state[q])
        for key in opt.state[p]:
            assert torch.equal(opt.state[p][key], opt2.state[q][key]), key


@pytest.mark.parametrize("name,kw", FULL)
def test_continues_from_a_state_dict_torch_stepped(A, name, kw):
    """torch.optim.<name> steps four times on the CPU (tensor 6 without a gradient); its own state_dict() -- no entry for tensor 6
    -- is loaded here, and ten more steps follow the torch run continued in float64."""
    start = _params(5)
    qs, ref = _oracle(name, start, kw)
    for step in range(4):
        _set64(qs, _grads(step, skip=_skip2(step)))
        ref.step()
    with torch.no_grad():                                      # what fp32 can hold: the two runs continue from the same numbers
        for q in qs:
            q.copy_(q.float().double())
            for key, val in ref.state.get(q, {}).items():
                if torch.is_tensor(val) and key != "step":
                    val.copy_(val.float().double())
    sd = copy.deepcopy(ref.state_dict())
    assert 6 not in sd["state"]
    ps = [torch.nn.Parameter(q.detach().float().cuda()) for q in qs]
    opt = getattr(A.optim, name)(ps, **kw)
    opt.load_state_dict(sd)
    for step in range(4, 14):
        gs = _grads(step, skip=_skip2(step))
        _set(ps, gs)
        _set64(qs, gs)
        opt.step()
        ref.step()
    torch.cuda.synchronize()
    _check_against(opt, ps, ref, qs, "from torch's state dict")
    if name == "RMSprop":
        assert float(opt.state[ps[6]]["step"]) == 8.0


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_trainer_fit_graph_on_and_off(A, name, precision):
    """EDSR with optimizer="SGD" / "RMSprop" through Trainer.fit, 10 steps, graph on and off: the same parameters.  fp16 trains under
    the device-resident loss scaler and still replays a graph."""
    from sr_amd import trainer as T
    out = []
    for use_graph in (True, False):
        torch.manual_seed(0)
        m = A.EDSR(scale_factor=2, precision=precision, n_feats=16, n_resblocks=2, res_scale=0.1, optimizer=name)
        tr = T.Trainer(device="cuda", use_graph=use_graph)
        tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 700 + i, "cpu") for i in range(10)))
        torch.cuda.synchronize()
        if use_graph:
            assert type(tr.graphed.opt) is getattr(A.optim, name)
        if precision == 16:
            assert tr.scaler is not None and hasattr(tr.scaler, "state")
        out.append((tr.losses, [p.detach().clone() for p in m.parameters()], tr.graphed))
    (lg, pg, g), (le, pe, _) = out
    assert g is not None and g.graphs is not None and not g.failed, "the step was captured"
    print(name, precision, "losses graphed", lg, "eager", le)
    assert len(lg) == len(le) == 10 and all(np.isfinite(lg))
    np.testing.assert_allclose(lg, le, rtol=2e-4 if precision == 32 else 2e-3)
    for a, b in zip(pg, pe):
        print(name, precision, tuple(a.shape), "max |diff| %.3e mean %.3e" % (float((a - b).abs().max()), float((a - b).abs().mean())))
        if precision == 32:
            assert float((a - b).abs().max()) <= 2e-4, float((a - b).abs().max())
        else:
            assert float((a - b).abs().max()) <= 9.5e-3 and float((a - b).abs().mean()) <= 3e-4
