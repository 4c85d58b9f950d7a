"""GPU tests of the device-side learning-rate schedules (csrc/lr_sched.hip through sr_amd.lr_sched.DeviceLRSchedule) and of the
optimizers' `lr_dev` path (csrc/optim.hip): the values against the float64 closed forms of lr_sched_ref.py, the four optimizers
reading the device value bit for bit like a twin that gets it by value, hipGraph replays that follow the schedule without a
re-capture, and Trainer.fit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lr_sched_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BASES = (2e-4, 1e-3)
SIZES = (3, 1025, 4101)          # a scalar tail only; one block with a 16-byte body and a tail; two blocks
# a step boundary at 7, 14, ...; the adjacent milestones 10 and 11; t == t_max at 25 and t > t_max after it; restarts at 8, 24 and 56
KINDS = [("constant", dict()), ("step", dict(step_size=7, gamma=0.5)), ("multistep", dict(milestones=[10, 11, 30], gamma=0.3)),
         ("cosine", dict(t_max=25, eta_min=1e-7)), ("cosine_restarts", dict(t_0=8, t_mult=2, eta_min=1e-7)),
         ("cosine_restarts", dict(t_0=7, t_mult=1, eta_min=0.0))]
WARMUPS = [dict(), dict(warmup_steps=9, warmup_start=0.1)]
OPTIMIZERS = [("Adam", dict()), ("Ranger", dict(k=3)), ("SGD", dict()), ("SGD", dict(momentum=0.9, nesterov=True)),
              ("RMSprop", dict()), ("RMSprop", dict(centered=True, momentum=0.5))]
OPT_IDS = ["Adam", "Ranger", "SGD", "SGD-nesterov", "RMSprop", "RMSprop-centered-momentum"]
# every step has another learning rate than the step before it, and a restart (step 4) lies inside the 12 steps
MOVING = ("cosine_restarts", dict(t_0=4, t_mult=2, eta_min=1e-7, warmup_steps=3, warmup_start=0.2))


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.rand(n, generator=g) - 0.5).cuda()) for n in SIZES]


def _grads(step):
    g = torch.Generator().manual_seed(1000 + step)
    return [(torch.rand(n, generator=g) - 0.5) * 10.0 ** (i % 3 - 1) for i, n in enumerate(SIZES)]


def _make(A, name, kw, ps, groups=2):
    if groups == 1:
        return getattr(A.optim, name)([{"params": ps, "lr": BASES[0]}], **kw)
    return getattr(A.optim, name)([{"params": ps[:2], "lr": BASES[0]}, {"params": ps[2:], "lr": BASES[1]}], **kw)


def _close(got, want, bases, what):
    assert len(got) == len(want) == len(bases)
    for g, w, b in zip(got, want, bases):
        assert abs(g - w) <= R.TOL * b, (what, g, w, abs(g - w) / b)


def _assert_same_bits(oa, pa, ob, pb):
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach()), a.shape
        assert set(oa.state[a]) == set(ob.state[b])
        for key in oa.state[a]:
            assert torch.equal(oa.state[a][key], ob.state[b][key]), (key, a.shape)


# ---- values ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", WARMUPS, ids=["plain", "warmup"])
@pytest.mark.parametrize("kind,consts", KINDS, ids=["constant", "step", "multistep", "cosine", "restarts-8x2", "restarts-7x1"])
def test_device_values_follow_the_closed_forms(A, kind, consts, warm):
    """SET(0), then 60 ADVANCEs: the device values and the host mirror against the float64 closed forms, on two groups."""
    kw = dict(consts, **warm)
    sched = A.lr_sched.DeviceLRSchedule(_make(A, "SGD", {}, _params(0)), kind, **kw)
    assert sched.on_gpu
    worst = 0.0
    for t in range(61):
        want = [R.lr(kind, t, b, **kw) for b in BASES]
        got = sched.device_lr()
        worst = max([worst] + [abs(g - w) / b for g, w, b in zip(got, want, BASES)])
        _close(got, want, BASES, (kind, "device", t))
        _close(sched.get_last_lr(), want, BASES, (kind, "host mirror", t))
        if t < 60:
            sched.step()
    print(f"{kind} {kw}: worst |device - float64| / base = {worst:.3g}")
    assert sched.count == 60 == sched.device_count()


def test_set_to_a_count_past_a_restart_gives_what_advance_reaches(A):
    kind, kw = "cosine_restarts", dict(t_0=8, t_mult=2, eta_min=1e-7, warmup_steps=9, warmup_start=0.1)
    walked = A.lr_sched.DeviceLRSchedule(_make(A, "SGD", {}, _params(0)), kind, **kw)
    for _ in range(30):
        walked.step()
    jumped = A.lr_sched.DeviceLRSchedule(_make(A, "SGD", {}, _params(0)), "constant")
    jumped.load_state_dict(dict(walked.state_dict(), count=30))
    assert jumped.device_lr() == walked.device_lr(), "SET(30) and 30 ADVANCEs: the same bits"
    assert jumped.device_count() == 30
    _close(jumped.device_lr(), [R.lr(kind, 30, b, **kw) for b in BASES], BASES, "SET(30)")
    jumped.step()
    walked.step()
    assert jumped.device_lr() == walked.device_lr()
    # past the third restart (56), and far out: the integer loop, not a logarithm
    for count in (56, 57, 8 * (2 ** 20 - 1)):
        jumped.load_state_dict(dict(walked.state_dict(), count=count))
        _close(jumped.device_lr(), [R.lr(kind, count, b, **kw) for b in BASES], BASES, count)


# ---- the optimizers read the device value -------------------------------------------------------------------------------------------------
def _twin_run(A, name, kw, groups, scaled, inf_at=None, steps=12):
    """`steps` steps of an optimizer with a schedule and of a twin that gets, by value before each step, exactly the double read back
    from the device.  Returns both and the learning rates every step used."""
    pa, pb = _params(1), _params(1)
    oa, ob = _make(A, name, kw, pa, groups), _make(A, name, kw, pb, groups)
    sched = A.lr_sched.DeviceLRSchedule(oa, MOVING[0], **MOVING[1])
    sa = A.optim.DeviceGradScaler("cuda") if scaled else None
    sb = A.optim.DeviceGradScaler("cuda") if scaled else None
    used = []
    for t in range(steps):
        lrs = sched.device_lr()
        used.append(lrs)
        assert [g["lr"] for g in oa.param_groups] == list(BASES[:groups]), "group['lr'] stays at the base value"
        for g, v in zip(ob.param_groups, lrs):
            g["lr"] = v
        scale = sa.get_scale() if scaled else 1.0
        for i, (p, q, g) in enumerate(zip(pa, pb, _grads(t))):
            g = g * scale
            if t == inf_at and i == len(pa) - 1:
                g[-1] = float("inf")                         # the last element of the last tensor of the last group
            p.grad, q.grad = g.cuda(), g.cuda()
        if scaled:
            oa.step(grad_scaler=sa)
            ob.step(grad_scaler=sb)
        else:
            oa.step()
            ob.step()
    torch.cuda.synchronize()
    return (oa, pa, sa), (ob, pb, sb), sched, used


@pytest.mark.parametrize("name,kw", OPTIMIZERS, ids=OPT_IDS)
def test_optimizers_read_lr_from_the_device(A, name, kw):
    (oa, pa, _), (ob, pb, _), sched, used = _twin_run(A, name, kw, 2, False)
    _assert_same_bits(oa, pa, ob, pb)
    assert all(a != b for a, b in zip(used, used[1:])), "every step had another learning rate than the one before"
    for t, lrs in enumerate(used):
        _close(lrs, [R.lr(MOVING[0], t, b, **MOVING[1]) for b in BASES], BASES, t)
    assert sched.device_count() == 12
    q = _params(1)
    assert all(not torch.equal(a.detach(), b.detach()) for a, b in zip(pa, q)), "the parameters moved"


@pytest.mark.parametrize("groups", [1, 2], ids=["combined-entry", "check-update-split"])
@pytest.mark.parametrize("name,kw", OPTIMIZERS, ids=OPT_IDS)
def test_optimizers_read_lr_from_the_device_under_the_loss_scaler(A, name, kw, groups):
    """One non-finite gradient at step 5: the update is skipped on the device, the schedule still advances (a skipped step is a call of
    step(), as in `scaler.step; scaler.update; scheduler.step`), and the twin does the same."""
    (oa, pa, sa), (ob, pb, sb), sched, used = _twin_run(A, name, kw, groups, True, inf_at=5)
    _assert_same_bits(oa, pa, ob, pb)
    assert sa.skipped_steps == sb.skipped_steps == 1 and sa.get_scale() == sb.get_scale() == 32768.0
    assert sched.device_count() == 12 == sched.count
    bases = BASES[:groups]
    assert used[5] != used[6]
    _close(used[6], [R.lr(MOVING[0], 6, b, **MOVING[1]) for b in bases], bases, "the step after the skipped one")


def test_by_value_lr_is_still_range_checked_and_lr_dev_lifts_it(A):
    ps = _params(2)
    opt = _make(A, "Ranger", {}, ps, 1)
    for p, g in zip(ps, _grads(0)):
        p.grad = g.cuda()
    opt.param_groups[0]["lr"] = 0.0
    with pytest.raises(RuntimeError, match="lr=0"):
        opt.step()                                            # by value: Ranger's launcher refuses lr <= 0
    sched = A.lr_sched.DeviceLRSchedule(opt, "manual")
    opt.step()                                               # from the device: the by-value field is not looked at
    sched.detach()
    assert opt._lr_dev is None and opt.lr_schedule is None and opt.param_groups[0]["lr"] == 0.0


# ---- replay ---------------------------------------------------------------------------------------------------------------------------------
def _replay_run(A, name, kw, graphed, kind, consts, steps, between=None):
    """Two eager steps, then `steps` more: eager, or one step captured (ops.graph_capture) and replayed on gradients rewritten in place."""
    ps = _params(3)
    opt = _make(A, name, kw, ps)
    sched = A.lr_sched.DeviceLRSchedule(opt, kind, **consts)
    static = [torch.zeros_like(p) for p in ps]
    for p, s in zip(ps, static):
        p.grad = s
    graph, captures = None, 0
    for t in range(2 + steps):
        for s, g in zip(static, _grads(t)):
            s.copy_(g)
        if between is not None:
            between(t, sched, opt)
        if not graphed or t < 2:
            opt.step()
            continue
        if graph is None:
            opt.reserve_capture_tables()
            graph = torch.cuda.CUDAGraph()
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                with A.ops.graph_capture(graph, stream=st):
                    opt.step()
            torch.cuda.current_stream().wait_stream(st)
            captures += 1
        graph.replay()
        sched.replayed()
    torch.cuda.synchronize()
    out = (opt, ps, sched, sched.device_lr(), sched.get_last_lr(), sched.device_count(), captures)
    if graph is not None:
        del graph
        opt.release_captured_tables()
    return out


@pytest.mark.parametrize("name,kw", [OPTIMIZERS[0], OPTIMIZERS[1], OPTIMIZERS[3], OPTIMIZERS[5]], ids=["Adam", "Ranger", "SGD-nesterov", "RMSprop-centered-momentum"])
def test_replayed_step_follows_the_schedule(A, name, kw):
    """One captured step, replayed 20 times: the parameters, the state and the device learning rates of 20 eager steps, bit for bit."""
    oe, pe, _, lre, hoste, ce, _ = _replay_run(A, name, kw, False, *MOVING, steps=20)
    og, pg, sched, lrg, hostg, cg, captures = _replay_run(A, name, kw, True, *MOVING, steps=20)
    assert captures == 1 and ce == cg == 22
    _assert_same_bits(oe, pe, og, pg)
    assert lre == lrg and hoste == hostg
    _close(lrg, [R.lr(MOVING[0], 22, b, **MOVING[1]) for b in BASES], BASES, "after 20 replays")
    _close(hostg, [R.lr(MOVING[0], 22, b, **MOVING[1]) for b in BASES], BASES, "host mirror after 20 replays")


def test_manual_set_lr_between_two_replays_needs_no_recapture(A):
    """kind="manual": `set_lr` between replays changes the next replay's update; the twin is an eager optimizer whose lr is set by hand."""
    def drive(t, sched, opt):
        if t == 4:
            sched.set_lr([5e-3, 7e-3])
        if t == 6:
            sched.set_lr(1e-5)
    og, pg, sched, lrg, hostg, count, captures = _replay_run(A, "SGD", dict(momentum=0.9), True, "manual", {}, steps=6, between=drive)
    assert captures == 1 and count == 8 and lrg == hostg == [1e-5, 1e-5]
    pt = _params(3)
    twin = _make(A, "SGD", dict(momentum=0.9), pt)
    for t in range(8):
        if t == 4:
            twin.param_groups[0]["lr"], twin.param_groups[1]["lr"] = 5e-3, 7e-3
        if t == 6:
            twin.param_groups[0]["lr"] = twin.param_groups[1]["lr"] = 1e-5
        for p, g in zip(pt, _grads(t)):
            p.grad = g.cuda()
        twin.step()
    _assert_same_bits(og, pg, twin, pt)
    with pytest.raises(RuntimeError, match="manual"):
        A.lr_sched.DeviceLRSchedule(_make(A, "SGD", {}, _params(0)), "constant").set_lr(1e-3)


# ---- Trainer.fit -----------------------------------------------------------------------------------------------------------------------------
# The smallest model and batch tests/test_gpu_trainer_graph.py trains (EDSR x2, 32 features, 2 blocks, 8 patches of 24x24).  Bit-for-bit
# comparisons of two training runs run in bf16, train.py's default precision: the weight gradients are summed in slab order
# (include/srk.h: "bitwise reproducible"), so a run repeats itself bit for bit.  When these tests were written the fp32 weight gradient
# (csrc/conv_wgrad.hip) still accumulated with float atomics, so fp32 is checked here for everything but the bits of the weights; it
# writes slabs now, and tests/test_gpu_step_reproducible.py holds fp32 runs to their bits.
def _fit(A, use_graph, optimizer, first, last, state=None, weights=None, precision="bf16"):
    """Trainer.fit over batches [first, last), lr halving every second step."""
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision=precision, n_feats=32, n_resblocks=2, res_scale=0.1, optimizer=optimizer,
               lr_schedule="step", lr_schedule_params=["step_size=2", "gamma=0.5"])
    if weights is not None:
        m.load_state_dict(weights)
    m.lr_schedule_state = state
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 300 + i, "cpu") for i in range(first, last)))
    torch.cuda.synchronize()
    return m, tr


@pytest.fixture(scope="module")
def fits(A):
    return {use_graph: _fit(A, use_graph, "ADAM", 0, 12) for use_graph in (True, False)}


def _check_schedule_after_12_steps(tr):
    sched = tr.optimizer.lr_schedule
    assert sched.on_gpu and tr.optimizer.param_groups[0]["lr"] == 1e-3, "group['lr'] stays at the base value"
    assert sched.count == 12 == sched.device_count()
    want = [R.lr("step", 12, 1e-3, step_size=2, gamma=0.5)]
    _close(sched.get_last_lr(), want, [1e-3], "get_last_lr")
    _close(sched.device_lr(), want, [1e-3], "device_lr")


def test_trainer_follows_the_schedule_with_one_capture(A, fits):
    """12 steps, lr halves every second step: five changes after the capture (step 3) and no re-capture; the host mirror and the device
    agree on the count and on the reference's value at count 12, replayed and launch by launch."""
    g = fits[True][1].graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step was captured"
    assert g.captures == 1
    assert fits[False][1].graphed is None
    for _, tr in fits.values():
        _check_schedule_after_12_steps(tr)


def test_trainer_fp32_follows_the_schedule_with_one_capture(A):
    _, tr = _fit(A, True, "ADAM", 0, 12, precision=32)
    g = tr.graphed
    assert g is not None and g.graphs is not None and not g.failed and g.captures == 1
    _check_schedule_after_12_steps(tr)


def test_trainer_replays_are_the_eager_loop_bit_for_bit(A, fits):
    """The per-step losses and the final parameters of the replayed loop and of `use_graph=False` with the same schedule: the same bits."""
    (mg, tg), (me, te) = fits[True], fits[False]
    diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(mg.parameters(), me.parameters()))
    print(f"graph against eager: losses {tg.losses} / {te.losses}; max |parameter difference| {diff:.3g}")
    assert len(tg.losses) == len(te.losses) == 12
    assert tg.losses == te.losses
    for a, b in zip(mg.parameters(), me.parameters()):
        assert torch.equal(a.detach(), b.detach())


def test_trainer_schedule_reaches_the_replays(A, fits):
    """The same 12 replayed steps at a constant learning rate end somewhere else."""
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision="bf16", n_feats=32, n_resblocks=2, res_scale=0.1)
    tr = T.Trainer(device="cuda", use_graph=True)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 300 + i, "cpu") for i in range(12)))
    torch.cuda.synchronize()
    assert tr.optimizer.lr_schedule is None and tr.graphed.captures == 1
    scheduled = fits[True][1].losses
    # steps 0 and 1 are updated at the base learning rate in both runs, so the losses of steps 0, 1 and 2 are the same numbers; the
    # update of step 2 is the first at half the rate.  By step 11 the scheduled run has moved 1 + 1 + 1/2 + 1/2 + ... = 3.9 base-lr
    # steps of Adam, the constant one 11
    assert tr.losses[:3] == scheduled[:3]
    assert all(a != b for a, b in zip(tr.losses[3:], scheduled[3:])), (tr.losses, scheduled)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_trainer_schedule_state_round_trip_at_step_6(A, use_graph):
    """Six steps, the schedule's state_dict, six more steps of a new optimizer and schedule that load it: the final parameters of
    twelve steps in one go, bit for bit.  (SGD without momentum: the schedule is the only state the optimizer carries over.)"""
    whole, _ = _fit(A, use_graph, "SGD", 0, 12)
    half, tr = _fit(A, use_graph, "SGD", 0, 6)
    sd = tr.optimizer.lr_schedule.state_dict()
    assert sd["count"] == 6 and sd["kind"] == "step"
    rest, tr2 = _fit(A, use_graph, "SGD", 6, 12, state=sd, weights=half.state_dict())
    assert tr2.optimizer.lr_schedule.device_count() == 12
    assert any(not torch.equal(a.detach(), b.detach()) for a, b in zip(half.parameters(), rest.parameters())), "the second half trained"
    for a, b in zip(whole.parameters(), rest.parameters()):
        assert torch.equal(a.detach(), b.detach())
