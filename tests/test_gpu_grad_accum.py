"""GPU tests of gradient accumulation (csrc/grad_accum.hip through sr_amd.grad_accum.GradAccum): SRK_ACCUM_ADD / SRK_ACCUM_FINAL bit
for bit against the fp32 restatement of grad_accum_ref.py (block boundaries, the unaligned scalar path, one and two parameter groups),
the four optimizers against a twin that is handed the host-folded gradient (also with a clipper and under the device loss scaler), a
non-finite micro-step, both phases as hipGraph replays, and Trainer.fit with one graph per phase.

Every comparison of the kernel is exact: the rule is three fp32 operations in a pinned order, and numpy's float32 arithmetic restates it."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_accum_ref as R  # noqa: E402
import test_gpu_grad_clip as GC  # noqa: E402  (its sizes, parameters, host gradients and the unaligned gradient view)
import test_gpu_lr_sched as LR  # noqa: E402  (its OPTIMIZERS list and bit comparison)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, VIEW, SCALE = GC.SIZES, GC.VIEW, GC.SCALE
SENTINEL = 123.0


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _set_grads(ps, arrays):
    """Fresh gradient tensors; tensor VIEW's is a view that starts at an odd element of a larger storage filled with a sentinel."""
    for i, (p, a) in enumerate(zip(ps, arrays)):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if i == VIEW:
            big = torch.full((t.numel() + 3,), SENTINEL, device="cuda")
            p.grad = big[1:1 + t.numel()]
            p.grad.copy_(t)
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = t.cuda()


def _acc_of(opt, accum, ps):
    """The accumulator's slice of every parameter that gets gradients, from the optimizer's plans."""
    out = []
    for p in ps:
        gi = next(i for i, g in enumerate(opt.param_groups) if any(q is p for q in g["params"]))
        off = opt._plans[gi].offsets[p]
        out.append(accum.acc(gi)[off:off + p.numel()].cpu().numpy())
    return out


def _window(w, k, mag=1.0):
    return [GC._host_grads(10 * w + j, mag) for j in range(k)]


def _fold(micro):
    """Per tensor the final gradient of a window (`micro`: per micro-step the list of arrays)."""
    return [R.window_f32([m[i] for m in micro]) for i in range(len(micro[0]))]


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("groups", [1, 2], ids=["one-group", "two-groups"])
def test_add_and_final_are_the_fp32_restatement(A, groups, k):
    ps, extra = GC._params(0)
    opt = GC._make(A, "SGD", {}, ps, extra, groups)
    accum = A.grad_accum.GradAccum(opt, k)
    assert accum.on_gpu and accum.inv_k == float(R.inv_k(k))
    before = [p.detach().clone() for p in ps]
    for w in range(2):
        micro = _window(w, k)
        want = [np.zeros(n, dtype=np.float32) for n in SIZES]
        for j in range(k - 1):
            _set_grads(ps, micro[j])
            assert accum.phase == "accumulate" and accum.step() is False and accum.pos == j + 1
            want = [R.add_f32(a, g) for a, g in zip(want, micro[j])]
            for a, b in zip(_acc_of(opt, accum, ps), want):
                assert np.array_equal(a, b), "acc after ADD"
            for g, b in zip(GC._read_grads(ps), micro[j]):
                assert np.array_equal(g, b), "ADD does not write the gradient"
            assert ps[VIEW].grad._base[0] == SENTINEL and bool((ps[VIEW].grad._base[-2:] == SENTINEL).all())
        for p, b in zip(ps, before):
            assert torch.equal(p.detach(), b), "nothing stepped inside the window"
        _set_grads(ps, micro[k - 1])
        assert accum.phase == "step" and accum.step() is True and accum.pos == 0
        for g, b in zip(GC._read_grads(ps), _fold(micro)):
            assert g.dtype == np.float32 and np.array_equal(g, b), "g after FINAL"
        for i, g in enumerate(GC._read_grads(ps)):
            per = [m[i] for m in micro]
            assert (np.abs(g.astype(np.float64) - R.window_f64(per)) <= R.bound(per)).all()
        for a in _acc_of(opt, accum, ps):
            assert not a.any(), "FINAL zeroes acc"
        for gi in range(groups):
            assert not bool(accum.acc(gi).any()), "and touches nothing else of it"
        base = ps[VIEW].grad._base
        assert base[0] == SENTINEL and bool((base[-2:] == SENTINEL).all()), "the storage around the view is untouched"
        assert extra.grad is None
        assert all(not torch.equal(p.detach(), b) for p, b in zip(ps, before)), "the window's step moved the parameters"
        before = [p.detach().clone() for p in ps]


# ---- twin optimizers ------------------------------------------------------------------------------------------------------------------
def _twins(A, name, kw, groups, k, clip, scaled, windows=3, bad_first=None):
    (pa, ea), (pb, eb) = GC._params(2), GC._params(2)
    oa, ob = GC._make(A, name, kw, pa, ea, groups), GC._make(A, name, kw, pb, eb, groups)
    sa = A.optim.DeviceGradScaler("cuda") if scaled else None
    sb = A.optim.DeviceGradScaler("cuda") if scaled else None
    scale = np.float32(SCALE if scaled else 1.0)
    accum = A.grad_accum.GradAccum(oa, k)
    if clip:
        val = GC._f32(GC.R.total_norm(GC._host_grads(0)) / 4)
        ca, cb = A.grad_clip.GradClip(oa, val), A.grad_clip.GradClip(ob, val)
    for w in range(windows):
        micro = [[a * scale for a in g] for g in _window(w, k, mag=1.0 + w)]
        if bad_first is not None and w == 0:
            micro[0][-1][-1] = np.float32(bad_first)
        for j in range(k):
            _set_grads(pa, micro[j])
            assert accum.step(grad_scaler=sa) == (j == k - 1)
        _set_grads(pb, _fold(micro))
        ob.step(grad_scaler=sb) if scaled else ob.step()
        if bad_first is not None and w == 0:
            yield oa, pa + [ea], sa, accum
    torch.cuda.synchronize()
    LR._assert_same_bits(oa, pa + [ea], ob, pb + [eb])
    fresh, _ = GC._params(2)
    assert all(not torch.equal(a.detach(), b.detach()) for a, b in zip(pa, fresh)), "the parameters moved"
    if clip:
        assert ca.stats() == cb.stats() and ca.stats()["num_clipped"] == windows, "one norm per window, of the mean gradient"
    if scaled:
        assert sa.skipped_steps == sb.skipped_steps == (0 if bad_first is None else 1)
        assert sa.get_scale() == sb.get_scale() == (SCALE if bad_first is None else SCALE / 2)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clipped"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name,kw", LR.OPTIMIZERS, ids=LR.OPT_IDS)
def test_each_optimizer_steps_on_the_window_mean(A, name, kw, k, clip):
    list(_twins(A, name, kw, 2, k, clip, False))


@pytest.mark.parametrize("groups", [1, 2], ids=["combined-entry", "check-update-split"])
@pytest.mark.parametrize("name,kw", LR.OPTIMIZERS, ids=LR.OPT_IDS)
def test_each_optimizer_under_the_loss_scaler(A, name, kw, groups):
    list(_twins(A, name, kw, groups, 3, False, True))


@pytest.mark.parametrize("bad", ["inf", "nan"])
@pytest.mark.parametrize("groups", [1, 2], ids=["combined-entry", "check-update-split"])
def test_non_finite_micro_step_skips_the_whole_window(A, groups, bad):
    """A non-finite element in the FIRST micro-step reaches the final gradient: nothing is updated, the scale halves once, FINAL still
    zeroes acc, and the next windows step like the twin's."""
    start, e0 = GC._params(2)
    run = _twins(A, "Adam", {}, groups, 3, False, True, bad_first=bad)
    oa, pa, sa, accum = next(run)
    for p, r in zip(pa, start + [e0]):
        assert torch.equal(p.detach(), r.detach()), "the window's update was skipped"
    for p in pa[:-1]:
        assert float(oa.state[p]["step"]) == 0.0 and not bool(oa.state[p]["exp_avg"].any()) and not bool(oa.state[p]["exp_avg_sq"].any())
    assert sa.skipped_steps == 1 and sa.get_scale() == SCALE / 2
    last = pa[-2].grad[-1].item()
    assert np.isnan(last) if bad == "nan" else last == float("inf")
    for gi in range(groups):
        assert not bool(accum.acc(gi).any()), "acc was zeroed although the window held a non-finite value"
    assert list(run) == []                                   # the remaining windows and the comparison with the twin


# ---- replay ---------------------------------------------------------------------------------------------------------------------------
def _replay_run(A, name, kw, graphed, k=3, windows=5):
    """One eager window, then `windows - 1` more: eager on fresh gradient tensors, or one graph per phase captured when the phase first
    comes up and replayed on gradients rewritten in place.  An EMA and an lr schedule hang on the optimizer's step hooks."""
    from sr_amd import trainer as T
    ps, extra = GC._params(4)
    opt = GC._make(A, name, kw, ps, extra, 2)
    sched = A.lr_sched.DeviceLRSchedule(opt, "step", step_size=2, gamma=0.5)
    ema = A.ema.ParamEMA(ps + [extra], 0.9)
    hook = T.EmaAfterStep(opt, ema)
    accum = A.grad_accum.GradAccum(opt, k)
    graphs = {}
    for w in range(windows):
        micro = _window(w, k)
        for j in range(k):
            if graphed and w == 1 and j == 0:
                _set_grads(ps, [np.zeros(n, dtype=np.float32) for n in SIZES])      # the static gradients from here on
            if not graphed or w == 0:
                _set_grads(ps, micro[j])
                accum.step()
                continue
            for p, a in zip(ps, micro[j]):
                p.grad.copy_(torch.from_numpy(a))
            phase = accum.phase
            assert phase == ("step" if j == k - 1 else "accumulate")
            if phase not in graphs:
                opt.reserve_capture_tables()
                g = graphs[phase] = torch.cuda.CUDAGraph()
                st = torch.cuda.Stream()
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    with A.ops.graph_capture(g, stream=st):
                        assert accum.step() == (phase == "step")
                torch.cuda.current_stream().wait_stream(st)
                assert accum.phase == phase, "under capture the host position does not advance"
            graphs[phase].replay()
            accum.replayed()
            if phase == "step":
                sched.replayed()
    torch.cuda.synchronize()
    out = (opt, ps + [extra], ema.num_updates, sched.count, sched.device_count(), sched.device_lr(), ema.flat.clone(), len(graphs), accum.pos)
    hook.remove()
    if graphs:
        graphs.clear()
        opt.release_captured_tables()
    return out


@pytest.mark.parametrize("name,kw", [("Adam", dict()), ("SGD", dict(momentum=0.9, nesterov=True))], ids=["Adam", "SGD-nesterov"])
def test_replayed_phases_follow_the_eager_sequence(A, name, kw):
    oe, pe, ne, ce, de, le, fe, _, _ = _replay_run(A, name, kw, False)
    og, pg, ng, cg, dg, lg, fg, captured, pos = _replay_run(A, name, kw, True)
    assert captured == 2 and pos == 0
    LR._assert_same_bits(oe, pe, og, pg)
    assert ne == ng == 5, "the EMA was updated once per window"
    assert ce == cg == de == dg == 5, "the schedule advanced once per window (host mirror and device count)"
    assert le == lg and torch.equal(fe, fg)


# ---- Trainer.fit ----------------------------------------------------------------------------------------------------------------------
BATCHES = 12


def _fit(A, use_graph, k):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision="bf16", n_feats=32, n_resblocks=2, res_scale=0.1, accumulate_grad_batches=k, lr_schedule="constant")
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(4, 3, 16, 2, 500 + i, "cpu") for i in range(BATCHES)))
    torch.cuda.synchronize()
    return m, tr


@pytest.mark.parametrize("k", [2, 3])
def test_trainer_keeps_one_graph_per_phase(A, k):
    (mg, tg), (me, te) = _fit(A, True, k), _fit(A, False, k)
    g = tg.graphed
    assert g is not None and not g.failed and g.captures == 2 and set(g.by_phase) == {"accumulate", "step"}
    assert te.graphed is None
    for tr in (tg, te):
        assert tr.optimizer.lr_schedule.device_count() == BATCHES // k == tr.optimizer.lr_schedule.count
        assert tr.optimizer._accum.pos == 0
    lg, le = tg.losses, te.losses
    assert len(lg) == len(le) == BATCHES
    assert lg[:k] == le[:k], "the first window runs the same eager code on the same weights"
    np.testing.assert_allclose(lg, le, rtol=2e-3)
    # the standard of test_gpu_trainer_graph.py::test_trainer_graph_replay_follows_the_eager_loop
    worst = max(float((a - b).abs().max()) for a, b in zip(mg.parameters(), me.parameters()))
    print(f"k={k}: max |graph - eager| over the parameters {worst:.3g}")
    for a, b in zip(mg.parameters(), me.parameters()):
        assert float((a - b).abs().max()) <= 9.5e-3 and float((a - b).abs().mean()) <= 3e-4


def test_trainer_without_accumulation_still_captures_once(A):
    m, tr = _fit(A, True, 1)
    assert tr.optimizer._accum is None and tr.graphed.accum is None and tr.graphed.by_phase == {}
    assert tr.graphed.captures == 1 and tr.graphed.graphs is not None and not tr.graphed.failed
    assert tr.optimizer.lr_schedule.device_count() == BATCHES


# ---- several ranks: the optimizer-first graph form ------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


RANKS_WORKER = r"""
import os, sys, torch
sys.path.insert(0, {root!r})
import sr_amd
from sr_amd import trainer as T
rank, world, local = T.init_distributed("cuda", force=True)
dev = torch.device("cuda", local)
K, mode = {k}, {mode!r}
torch.manual_seed(0)
m = sr_amd.EDSR(n_feats=32, n_resblocks=2, res_scale=0.1, scale_factor=2, precision="bf16", accumulate_grad_batches=K, lr_schedule="constant").to(dev)
full = [T.synthetic_batch(4, 3, 16, 2, 600 + i, "cpu") for i in range(12)]
per = 4 // world
gs = T.GradSync(m, bucket_bytes=64 << 10)
gs.broadcast()
opt = m.configure_optimizers()[0]
gstep = T.GraphedStep(m, m, opt, gs, warm_steps=2 if mode == "graph" else 10 ** 9)
assert gstep.segments == 1
for b in full:
    gstep({{k: v[rank * per:(rank + 1) * per].to(dev) for k, v in b.items() if torch.is_tensor(v)}})
if mode == "graph":
    assert not gstep.failed and gstep.captures == 2 and set(gstep.by_phase) == {{"accumulate", "step"}}, (gstep.failed, gstep.captures)
    assert all(len(g) == 2 for g, _ in gstep.by_phase.values())
gstep.finish()
torch.cuda.synchronize()
assert opt._accum.pos == 0 and opt.lr_schedule.device_count() == 12 // K == opt.lr_schedule.count
torch.save({{k: v.float().cpu() for k, v in m.state_dict().items()}}, os.path.join({out!r}, f"{{mode}}_r{{rank}}.pt"))
torch.distributed.barrier()
torch.distributed.destroy_process_group()
"""


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [1, 2], ids=["one-rank-group", "two-ranks"])
def test_optimizer_first_graph_form_accumulates_like_its_eager_form(A, tmp_path, world):
    """`GraphedStep` over an `nccl` process group (the graph opens with the micro-step of the PENDING gradients, one graph per phase)
    against the same loop launch by launch.  One rank exercises the form itself; two ranks (where two devices are visible) also the
    replicas' equality."""
    if torch.cuda.device_count() < world:
        pytest.skip("needs two visible devices")
    k, sds = 3, {}
    for mode in ("graph", "eager"):
        script = tmp_path / f"worker_{mode}.py"
        script.write_text(RANKS_WORKER.format(root=ROOT, mode=mode, out=str(tmp_path), k=k))
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(v, None)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), str(script)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        sds[mode] = [torch.load(tmp_path / f"{mode}_r{r}.pt") for r in range(world)]
        for key in sds[mode][0]:
            for s in sds[mode][1:]:
                assert torch.equal(sds[mode][0][key], s[key]), f"replicas diverged at {key}"
    for key, v in sds["graph"][0].items():
        d = (v - sds["eager"][0][key]).abs()
        assert float(d.max()) <= 9.5e-3 and float(d.mean()) <= 3e-4, key
