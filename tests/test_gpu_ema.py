"""GPU tests of sr_amd.ema.ParamEMA (csrc/ema.hip: the exponential moving average of every parameter tensor, and its in-place
exchange with the weights, as one launch) against the float64 restatement in ema_ref.py: the update, the swap, hipGraph replay next to
an optimizer step, the device-resident loss scaler's skipped step, the models' caches across a swap, and Trainer.fit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ema_ref import EmaRef  # noqa: E402

pytestmark = pytest.mark.gpu

# one element; below a float4; a float4 and a tail; one block less one, exactly, plus one; two blocks and one element; nine blocks; a
# last block that is short and ends in a tail
SHAPES = [(1,), (3,), (5,), (4095,), (4096,), (4097,), (8193,), (64, 64, 3, 3), (33, 1000)]
OFFSET_N = 5000        # the parameter that starts one element into a larger storage: two blocks on the scalar path


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


def _params(seed):
    """SHAPES, then a slice that starts one element into its storage: 4-byte but not 16-byte aligned."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.rand(*s, generator=g) - 0.5).cuda()) for s in SHAPES]
    base = (torch.rand(OFFSET_N + 1, generator=g) - 0.5).cuda()
    off = torch.nn.Parameter(base[1:])
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    return ps + [off]


def _move(ps, step):
    """The parameters change by about 0.1 (uniform in +-0.1) per step."""
    g = torch.Generator().manual_seed(500 + step)
    with torch.no_grad():
        for p in ps:
            p.add_(((torch.rand(p.shape, generator=g) - 0.5) * 0.2).cuda())


def _grads(step, ps):
    g = torch.Generator().manual_seed(1000 + step)
    return [(torch.rand(p.shape, generator=g) - 0.5) * (10.0 ** (i % 4 - 2)) for i, p in enumerate(ps)]


def _np(ts):
    return [t.detach().double().cpu().numpy() for t in ts]


def _check(ema, ps, ref, what):
    worst = max(float(np.abs(ema.shadow(p).double().cpu().numpy() - s).max()) for p, s in zip(ps, ref.s))
    bound = ref.bound()
    print("%s: max |err| %.3e (bound %.3e = %d * 2^-21 * %.3f)" % (what, worst, bound, ref.count, ref.mag))
    assert worst <= bound, (what, worst, bound)


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_update_matches_the_restatement(A, decay):
    ps = _params(1)
    ps[2].requires_grad_(False)                               # averaged like the trainable ones
    ema = A.ema.ParamEMA(ps, decay)
    assert ema.on_gpu and ema.num_updates == 0
    for p in ps:
        assert torch.equal(ema.shadow(p), p.detach()) and ema.shadow(p).shape == p.shape
    ref = EmaRef(_np(ps), decay)
    for step in range(20):
        _move(ps, step)
        before = [p.detach().clone() for p in ps]
        ema.update()
        ref.update(_np(ps))
    torch.cuda.synchronize()
    assert ema.num_updates == ref.count == 20
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before)), "the update reads the parameters only"
    _check(ema, ps, ref, "decay %g" % decay)


def test_swap_store_load_are_bit_exact(A):
    ps = _params(2)
    ema = A.ema.ParamEMA(ps, 0.5)
    _move(ps, 0)
    ema.update()
    torch.cuda.synchronize()
    live = [p.detach().clone() for p in ps]
    avg = [ema.shadow(p).clone() for p in ps]
    assert all(not torch.equal(a, l) for a, l in zip(avg, live))
    vers = [p._version for p in ps]
    ema.swap()
    torch.cuda.synchronize()
    for p, a, l, v in zip(ps, avg, live, vers):
        assert torch.equal(p.detach(), a) and torch.equal(ema.shadow(p), l) and p._version > v, p.shape
    ema.swap()
    torch.cuda.synchronize()
    for p, a, l in zip(ps, avg, live):
        assert torch.equal(p.detach(), l) and torch.equal(ema.shadow(p), a), p.shape
    assert ema.num_updates == 1
    with pytest.raises(KeyError):
        with ema.swapped():
            assert torch.equal(ps[-1].detach(), avg[-1])
            raise KeyError("body")
    torch.cuda.synchronize()
    for p, a, l in zip(ps, avg, live):
        assert torch.equal(p.detach(), l) and torch.equal(ema.shadow(p), a), p.shape
    vers = [p._version for p in ps]
    ema.load()
    torch.cuda.synchronize()
    for p, a, v in zip(ps, avg, vers):
        assert torch.equal(p.detach(), a) and torch.equal(ema.shadow(p), a) and p._version > v, p.shape
    _move(ps, 1)
    ema.store()
    torch.cuda.synchronize()
    for p in ps:
        assert torch.equal(ema.shadow(p), p.detach()), p.shape
    # the padding between the tensors of the flat buffer was never written
    used = torch.zeros_like(ema.flat, dtype=torch.bool)
    for p in ps:
        o = ema._offsets[p]
        used[o:o + p.numel()] = True
    assert bool((ema.flat[~used] == 0).all())


def test_graph_replay_is_bit_identical_to_eager(A):
    """[opt.step(); ema.update()]: two eager steps, then captured and replayed 8 times on gradients rewritten in place; the decay
    changes before step 6 with no re-capture.  The eager twin runs the same kernels on the same inputs: the same bits."""
    runs = []
    traj = []
    for graphed in (False, True):
        ps = _params(3)
        opt = A.optim.Adam(ps, lr=1e-2)
        ema = A.ema.ParamEMA(ps, 0.9)
        static = [torch.zeros_like(p) for p in ps]
        for p, s in zip(ps, static):
            p.grad = s
        graph = None
        if not graphed:
            traj.append(_np(ps))
        for step in range(10):
            for s, g in zip(static, _grads(step, ps)):
                s.copy_(g)
            if step == 6:
                ema.set_decay(0.99)
            if not graphed or step < 2:
                opt.step()
                ema.update()
            else:
                if graph is None:
                    opt.reserve_capture_tables()
                    graph = torch.cuda.CUDAGraph()
                    st = torch.cuda.Stream()
                    st.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(st):
                        with torch.cuda.graph(graph, stream=st):
                            opt.step()
                            ema.update()
                    torch.cuda.current_stream().wait_stream(st)
                graph.replay()
            if not graphed:
                traj.append(_np(ps))
        torch.cuda.synchronize()
        runs.append((ps, ema))
        if graph is not None:
            del graph
            opt.release_captured_tables()
    (pe, ee), (pg, eg) = runs
    assert ee.num_updates == eg.num_updates == 10
    for a, b in zip(pe, pg):
        assert torch.equal(a.detach(), b.detach()), a.shape
        assert torch.equal(ee.shadow(a), eg.shadow(b)), a.shape
        assert not torch.equal(eg.shadow(b), b.detach())
    ref = EmaRef(traj[0], 0.9)
    for step in range(10):
        if step == 6:
            ref.set_decay(0.99)
        ref.update(traj[step + 1])
    _check(eg, pg, ref, "replayed")


def test_device_grad_scaler_skipped_step_still_updates(A):
    """The average follows every call of step() through the trainer's hook.  A step the scaler skips on the device leaves the
    parameters alone; the shadow moves towards them as the recurrence says, and the count advances."""
    from sr_amd import trainer as T
    ps = _params(4)
    opt = A.optim.Adam(ps, lr=1e-2)
    ema = A.ema.ParamEMA(ps, 0.9)
    scaler = A.optim.DeviceGradScaler(ps[0].device)
    hook = T.EmaAfterStep(opt, ema)
    ref = EmaRef(_np(ps), 0.9)
    scale = scaler.get_scale()
    for step in range(3):
        gs = _grads(step, ps)
        if step == 1:
            gs[7][3, 5, 1, 2] = float("inf")
        for p, g in zip(ps, gs):
            p.grad = (g * scale).cuda()
        before = [p.detach().clone() for p in ps]
        opt.step(grad_scaler=scaler)
        torch.cuda.synchronize()
        moved = [not torch.equal(p.detach(), b) for p, b in zip(ps, before)]
        assert (not any(moved)) if step == 1 else all(moved), (step, moved)
        ref.update(_np(ps))
        scale = scaler.get_scale()
    hook.remove()
    assert scaler.skipped_steps == 1 and ema.num_updates == ref.count == 3
    _check(ema, ps, ref, "scaler")
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt.step(grad_scaler=scaler)
    assert ema.num_updates == 3, "the hook is removed"


def _model(A, name, **extra):
    kw = {"EDSR": dict(n_feats=16, n_resblocks=2, res_scale=0.1, precision=32),
          "WDSR": dict(type="B", n_feats=64, n_resblocks=2, precision="bf16"),
          "SRResNet": dict(n_feats=16, n_resblocks=2, precision=32)}[name]
    return getattr(A, name)(scale_factor=2, **kw, **extra)


@pytest.mark.parametrize("name", ["EDSR", "WDSR", "SRResNet"])
def test_models_evaluate_under_the_average(A, name):
    """Whatever a model caches per weight (packed weights, folded constants, weight-norm effective weights) follows the swap: inside
    `ema_weights()` the output is, bit for bit, that of a fresh model loaded from `ema.state_dict(model)`, and afterwards the live
    weights' again."""
    torch.manual_seed(0)
    m = _model(A, name).cuda().eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, b in m.named_buffers():                        # BatchNorm statistics that are not the initial 0 / 1
            if k.endswith("running_mean"):
                b.add_((torch.rand(b.shape, generator=g) * 0.2 - 0.1).cuda())
            elif k.endswith("running_var"):
                b.add_((torch.rand(b.shape, generator=g) * 0.5).cuda())
    ema = m.make_ema(decay=0.9)
    batch = {"lr": torch.rand(1, 3, 24, 24, generator=g).cuda()}
    with torch.no_grad():
        m.predict_step(batch, 0)                              # every cache is warm with the initial weights
        for step in range(3):
            for p in (q for q in m.parameters() if q.requires_grad):      # (the frozen MeanShift weights stay the identity)
                p.add_((torch.randn(p.shape, generator=g) * 0.02).cuda() * p.abs().mean().clamp_min(0.05))
            ema.update()
        y_live = m.predict_step(batch, 0).clone()
        with m.ema_weights():
            y_ema = m.predict_step(batch, 0).clone()
        y_back = m.predict_step(batch, 0).clone()
        fresh = _model(A, name)
        fresh.load_state_dict(ema.state_dict(m), strict=True)
        y_fresh = fresh.cuda().eval().predict_step(batch, 0)
    torch.cuda.synchronize()
    assert ema.num_updates == 3 and bool(torch.isfinite(y_ema).all())
    assert not torch.equal(y_ema, y_live), "the average differs from the live weights"
    assert torch.equal(y_ema, y_fresh), float((y_ema - y_fresh).abs().max())
    assert torch.equal(y_back, y_live), float((y_back - y_live).abs().max())


@pytest.mark.parametrize("decay", [0.0, 1.0])
def test_trainer_fit_updates_behind_every_step(A, decay):
    """Nine steps at batch 2: three eager, the capture, replays.  Nine updates.  decay 0: the shadow is the final weights bit for bit,
    so the last update followed the last optimizer step; decay 1: the initial ones, so nothing else wrote the shadow."""
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = _model(A, "EDSR", ema_decay=decay).cuda()
    if decay == 0.0:
        m.make_ema(decay=0.0)                                 # (`ema_decay=0` is "off": an average made by hand, which fit() adopts)
    first = [p.detach().clone() for p in m.parameters()]
    tr = T.Trainer(device="cuda", use_graph=True)
    tr.fit(m, (T.synthetic_batch(2, 3, 24, 2, 900 + i, "cpu") for i in range(9)))
    torch.cuda.synchronize()
    g = tr.graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step was captured"
    assert len(tr.losses) == 9 and m.ema.num_updates == 9
    last = [p.detach() for p in m.parameters()]
    trainable = [i for i, p in enumerate(m.parameters()) if p.requires_grad]
    assert all(not torch.equal(first[i], last[i]) for i in trainable)
    want = last if decay == 0.0 else first
    for p, w in zip(m.parameters(), want):
        assert torch.equal(m.ema.shadow(p), w), tuple(p.shape)
