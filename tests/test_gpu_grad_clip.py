"""GPU tests of gradient clipping inside the optimizer step (csrc/grad_clip.hip through sr_amd.grad_clip.GradClip): the device norm and
coefficient against the float64 restatement of clip_ref.py, the clipped gradients bit for bit, the four optimizers against a twin that
is handed the already clipped gradients (also under the device loss scaler), non-finite gradients, hipGraph replays, and Trainer.fit.

Tolerances.  `total_norm` and `coef` are double results rounded ONCE to fp32 (relative error <= 2^-24); the double accumulation of
fewer than 2^15 squares adds less than 2^-30: the limit is a relative 2^-23.  The thresholds handed to the device are fp32-representable
numbers, so the reference uses exactly the threshold the kernel reads."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R  # noqa: E402
import test_gpu_lr_sched as LR  # noqa: E402  (its OPTIMIZERS list and bit comparison)

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -23
# a lone element, an unaligned tail, one short of a block, a full block, one over, several blocks with a tail
SIZES = (1, 3, 4095, 4096, 4097, 4 * 4096 + 5)
VIEW = 4                # this tensor's gradient is a view that starts at an odd element of a larger storage: the scalar paths
SCALE = 65536.0         # DeviceGradScaler's initial scale


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _params(seed):
    """The parameters that get gradients (SIZES) and one that never does."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.rand(n, generator=g) - 0.5).cuda()) for n in SIZES]
    return ps, torch.nn.Parameter((torch.rand(17, generator=g) - 0.5).cuda())


def _host_grads(step, mag=1.0):
    g = torch.Generator().manual_seed(2000 + step)
    return [((torch.rand(n, generator=g) - 0.5) * (10.0 ** (i % 3 - 1) * mag)).numpy() for i, n in enumerate(SIZES)]


def _set_grads(ps, arrays):
    for i, (p, a) in enumerate(zip(ps, arrays)):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if i == VIEW:
            big = torch.zeros(t.numel() + 3, device="cuda")
            p.grad = big[1:1 + t.numel()]
            p.grad.copy_(t)
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = t.cuda()


def _read_grads(ps):
    return [p.grad.detach().cpu().numpy() for p in ps]


def _make(A, name, kw, ps, extra, groups):
    if groups == 1:
        return getattr(A.optim, name)([{"params": ps[:2] + [extra] + ps[2:], "lr": 2e-4}], **kw)
    return getattr(A.optim, name)([{"params": ps[:2] + [extra] + ps[2:3], "lr": 2e-4}, {"params": ps[3:], "lr": 1e-3}], **kw)


def _f32(x):
    return float(np.float32(x))


def _rel(a, b):
    return abs(a - b) / abs(b)


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2], ids=["one-group", "two-groups"])
@pytest.mark.parametrize("factor", [0.25, 2.0], ids=["clips", "does-not-clip"])
def test_norm_coef_and_clipped_gradients(A, groups, factor):
    """max_norm = norm / 4 (clips) or 2 * norm (does not): the device norm and coefficient against float64; the gradients after the step
    are float32(g) * coef bit for bit (untouched when nothing clips), and their norm is back under the threshold."""
    ps, extra = _params(0)
    g0 = _host_grads(0)
    norm = R.total_norm(g0)
    max_norm = _f32(factor * norm)
    opt = _make(A, "SGD", {}, ps, extra, groups)
    clip = A.grad_clip.GradClip(opt, max_norm)
    assert clip.on_gpu and clip.partials.numel() == sum((n + 4095) // 4096 for n in SIZES) + 1
    _set_grads(ps, g0)
    opt.step()
    s = clip.stats()
    want_coef = R.coef(norm, max_norm)
    print(f"total_norm {s['total_norm']!r} (float64 {norm!r}, rel {_rel(s['total_norm'], norm):.3g}); coef {s['coef']!r} (float64 {want_coef!r}, "
          f"rel {_rel(s['coef'], want_coef):.3g})")
    assert _rel(s["total_norm"], norm) <= TOL
    assert _rel(s["coef"], want_coef) <= TOL
    assert float(clip.total_norm) == s["total_norm"] and float(clip.coef) == s["coef"] and clip.total_norm.dim() == 0
    assert s["num_clipped"] == (1 if factor < 1 else 0) and s["num_nonfinite"] == 0
    got = _read_grads(ps)
    if factor > 1:
        assert s["coef"] == 1.0
        for a, b in zip(got, g0):
            assert np.array_equal(a, b)
    else:
        assert s["coef"] < 1.0
        c = np.float32(s["coef"])
        for a, b in zip(got, g0):
            assert a.dtype == np.float32 and np.array_equal(a, b * c)
        after = R.total_norm(got)
        print(f"norm after clipping {after!r} / max_norm {max_norm!r} = {after / max_norm!r}")
        assert after <= max_norm * (1 + 2.0 ** -22)
    assert extra.grad is None


@pytest.mark.parametrize("groups", [1, 2], ids=["one-group", "two-groups"])
def test_value_clip_is_the_reference_clamp_and_keeps_nan(A, groups):
    ps, extra = _params(1)
    g0 = _host_grads(1)
    g0[3][77] = np.float32("nan")
    g0[VIEW][4096] = np.float32("nan")                        # in the scalar path's second block
    g0[5][5], g0[5][6] = np.float32("inf"), np.float32("-inf")
    bound = 0.03                                            # inside the range of every tensor but the smallest-magnitude ones
    opt = _make(A, "SGD", {}, ps, extra, groups)
    clip = A.grad_clip.GradClip(opt, bound, "value")
    _set_grads(ps, g0)
    opt.step()
    got, want = _read_grads(ps), R.clip_by_value(g0, bound)
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.isnan(got[3][77]) and np.isnan(got[VIEW][4096]) and got[5][5] == np.float32(bound) and got[5][6] == -np.float32(bound)
    assert sum(int(np.sum(a != b)) for a, b in zip(got, g0)) > 1000, "the bound cut something"
    assert clip.stats()["num_clipped"] == 0, "no norm launches"


def _twin_steps(A, name, kw, groups, algorithm, scaled, steps=3):
    """`steps` steps of an optimizer with a clipper and of a twin without one that is handed, before each step, the gradients clipped
    on the host with the coefficient read back from the device (value: the reference clamp).  Under the scaler the gradients carry the
    loss scale, and the twin receives the clipped and still scaled ones."""
    (pa, ea), (pb, eb) = _params(2), _params(2)
    oa, ob = _make(A, name, kw, pa, ea, groups), _make(A, name, kw, pb, eb, groups)
    sa = A.optim.DeviceGradScaler("cuda") if scaled else None
    sb = A.optim.DeviceGradScaler("cuda") if scaled else None
    scale = np.float32(SCALE if scaled else 1.0)
    val = 0.03 if algorithm == "value" else _f32(R.total_norm(_host_grads(0)) / 4)
    clip = A.grad_clip.GradClip(oa, val, algorithm)
    for t in range(steps):
        g = [a * scale for a in _host_grads(t, mag=1.0 + t)]       # (the norm grows: every step clips, by another coefficient)
        _set_grads(pa, g)
        oa.step(grad_scaler=sa) if scaled else oa.step()
        if algorithm == "norm":
            s = clip.stats()
            norm = R.total_norm(g, scale)
            assert _rel(s["total_norm"], norm) <= TOL, "the norm of the UNSCALED gradients"
            assert _rel(s["coef"], R.coef(norm, val)) <= TOL and s["coef"] < 1.0 and s["num_clipped"] == t + 1
            clipped = [a * np.float32(s["coef"]) for a in g]
        else:
            clipped = R.clip_by_value(g, np.float32(val) * scale)
        for a, b in zip(_read_grads(pa), clipped):
            assert np.array_equal(a, b), "p.grad holds the clipped (and still scaled) gradient"
        _set_grads(pb, clipped)
        ob.step(grad_scaler=sb) if scaled else ob.step()
    torch.cuda.synchronize()
    LR._assert_same_bits(oa, pa + [ea], ob, pb + [eb])
    fresh, _ = _params(2)
    assert all(not torch.equal(a.detach(), b.detach()) for a, b in zip(pa, fresh)), "the parameters moved"
    if scaled:
        assert sa.skipped_steps == sb.skipped_steps == 0 and sa.get_scale() == sb.get_scale() == SCALE


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("name,kw", LR.OPTIMIZERS, ids=LR.OPT_IDS)
def test_each_optimizer_steps_on_the_clipped_gradients(A, name, kw, algorithm):
    _twin_steps(A, name, kw, 2, algorithm, False)


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("groups", [1, 2], ids=["combined-entry", "check-update-split"])
@pytest.mark.parametrize("name,kw", LR.OPTIMIZERS, ids=LR.OPT_IDS)
def test_each_optimizer_under_the_loss_scaler(A, name, kw, groups, algorithm):
    _twin_steps(A, name, kw, groups, algorithm, True)


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("bad", ["inf", "nan"])
@pytest.mark.parametrize("groups", [1, 2], ids=["combined-entry", "check-update-split"])
def test_non_finite_gradient_under_the_scaler_skips_the_step(A, groups, bad, algorithm):
    """One non-finite element in the last tensor: the clipper leaves it where the scaler's check finds it, nothing is updated, the scale
    halves exactly as for a twin without a clipper.  By norm: coef is 1, `num_nonfinite` advances and every gradient is untouched.  (By
    value there are no norm launches, so there is no coefficient and nothing to count: the finite elements are clamped as usual.)"""
    (pa, ea), (pb, eb) = _params(3), _params(3)
    oa, ob = _make(A, "Adam", {}, pa, ea, groups), _make(A, "Adam", {}, pb, eb, groups)
    sa, sb = A.optim.DeviceGradScaler("cuda"), A.optim.DeviceGradScaler("cuda")
    clip = A.grad_clip.GradClip(oa, 1e-3 if algorithm == "norm" else 0.03, algorithm)
    g = [a * np.float32(SCALE) for a in _host_grads(0)]
    g[-1][-1] = np.float32(bad)
    _set_grads(pa, g)
    _set_grads(pb, g)
    oa.step(grad_scaler=sa)
    ob.step(grad_scaler=sb)
    start, _ = _params(3)
    for p, q, r in zip(pa, pb, start):
        assert torch.equal(p.detach(), r.detach()) and torch.equal(q.detach(), r.detach()), "the step was skipped"
    assert sa.skipped_steps == sb.skipped_steps == 1 and sa.get_scale() == sb.get_scale() == SCALE / 2
    s, got = clip.stats(), _read_grads(pa)
    last = got[-1][-1]
    assert np.isnan(last) if bad == "nan" else last == np.float32("inf")
    if algorithm == "norm":
        assert s["coef"] == 1.0 and s["num_nonfinite"] == 1 and s["num_clipped"] == 0 and not np.isfinite(s["total_norm"])
        for a, b in zip(got, g):
            assert np.array_equal(a, b, equal_nan=True)
    else:
        want = R.clip_by_value(g, np.float32(0.03) * np.float32(SCALE))
        want[-1][-1] = g[-1][-1]
        for a, b in zip(got, want):
            assert np.array_equal(a, b, equal_nan=True)
    # the next, finite step goes through and clips
    g = [a * np.float32(SCALE / 2) for a in _host_grads(1)]
    _set_grads(pa, g)
    oa.step(grad_scaler=sa)
    assert sa.skipped_steps == 1 and not torch.equal(pa[0].detach(), start[0].detach())
    if algorithm == "norm":
        s = clip.stats()
        assert s["num_clipped"] == 1 and s["num_nonfinite"] == 1 and _rel(s["total_norm"], R.total_norm(g, SCALE / 2)) <= TOL


# ---- replay -----------------------------------------------------------------------------------------------------------------------------------
# the norm of _host_grads(t, 1.0) is 412.6 .. 414.9 for every t: magnitude 1 lies 8x above the threshold 50, magnitude 0.05 at 0.41x
MAGS = (1.0, 0.05, 1.0, 0.05, 1.0, 1.0, 0.05, 1.0)
MAX_NORM, RAISED_AT, RAISED = 50.0, 5, 5000.0       # from step 5 on the threshold is 5000: nothing clips any more


def _replay_run(A, name, kw, graphed, scaled):
    """Two eager steps, then six more: eager on fresh gradient tensors, or one step captured and replayed on gradients rewritten in place."""
    ps, extra = _params(4)
    opt = _make(A, name, kw, ps, extra, 2)
    clip = A.grad_clip.GradClip(opt, MAX_NORM)
    sc = A.optim.DeviceGradScaler("cuda") if scaled else None
    step = (lambda: opt.step(grad_scaler=sc)) if scaled else opt.step
    scale = np.float32(SCALE if scaled else 1.0)
    if graphed:
        _set_grads(ps, [np.zeros(n, dtype=np.float32) for n in SIZES])        # the static gradients (one of them the unaligned view)
    graph, captures, coefs = None, 0, []
    for t, mag in enumerate(MAGS):
        g = [a * scale for a in _host_grads(t, mag)]
        if t == RAISED_AT:
            clip.set_clip_val(RAISED)
        if graphed:
            for p, a in zip(ps, g):
                p.grad.copy_(torch.from_numpy(a))
        else:
            _set_grads(ps, g)
        if not graphed or t < 2:
            step()
        else:
            if graph is None:
                opt.reserve_capture_tables()
                graph = torch.cuda.CUDAGraph()
                st = torch.cuda.Stream()
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    with A.ops.graph_capture(graph, stream=st):
                        step()
                torch.cuda.current_stream().wait_stream(st)
                captures += 1
            graph.replay()
        coefs.append(float(clip.coef))
    torch.cuda.synchronize()
    out = (opt, ps + [extra], clip.stats(), coefs, captures, _read_grads(ps))
    if graph is not None:
        del graph
        opt.release_captured_tables()
    return out


@pytest.mark.parametrize("name,kw,scaled", [("Adam", dict(), False), ("SGD", dict(momentum=0.9, nesterov=True), False), ("Adam", dict(), True)],
                         ids=["Adam", "SGD-nesterov", "Adam-scaled"])
def test_replayed_step_clips_like_the_eager_one(A, name, kw, scaled):
    """One capture, six replays on fresh gradient contents, some above the threshold and some below; `set_clip_val` between two replays
    takes effect without a re-capture.  Parameters, optimizer state, the counters and the clipped gradients: the eager twin's bits."""
    oe, pe, se, ce, _, ge = _replay_run(A, name, kw, False, scaled)
    og, pg, sg, cg, captures, gg = _replay_run(A, name, kw, True, scaled)
    assert captures == 1
    LR._assert_same_bits(oe, pe, og, pg)
    assert sg == se and cg == ce
    for a, b in zip(ge, gg):
        assert np.array_equal(a, b)
    norms = [R.total_norm(_host_grads(t, mag)) for t, mag in enumerate(MAGS)]
    limits = [MAX_NORM if t < RAISED_AT else RAISED for t in range(len(MAGS))]
    assert all(n >= 4 * m or n <= 0.5 * m for n, m in zip(norms, limits)), (norms, "no borderline step")
    want = [n > m for n, m in zip(norms, limits)]
    assert want == [True, False, True, False, True, False, False, False]
    assert [c < 1.0 for c in cg] == want and sg["num_clipped"] == sum(want) == 3 and sg["num_nonfinite"] == 0
    for c, n, m in zip(cg, norms, limits):
        assert _rel(c, R.coef(n, m)) <= TOL


# ---- Trainer.fit ------------------------------------------------------------------------------------------------------------------------------
# The smallest model and batch of the trainer tests, in bf16: test_gpu_lr_sched.py records why two fp32 runs are not bit-comparable.
STEPS = 8


def _fit(A, use_graph, clip_val):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision="bf16", n_feats=32, n_resblocks=2, res_scale=0.1, gradient_clip_val=clip_val)
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 300 + i, "cpu") for i in range(STEPS)))
    torch.cuda.synchronize()
    return m, tr


@pytest.fixture(scope="module")
def fits(A):
    return {key: _fit(A, *key) for key in ((True, 1e-3), (False, 1e-3), (True, None), (True, 1e9))}


def test_trainer_replays_clip_like_the_eager_loop_with_one_capture(A, fits):
    (mg, tg), (me, te) = fits[(True, 1e-3)], fits[(False, 1e-3)]
    g = tg.graphed
    assert g is not None and g.graphs is not None and not g.failed and g.captures == 1, "the step was captured once"
    assert te.graphed is None
    for tr in (tg, te):
        s = tr.optimizer._clip.stats()
        print(f"clip stats after {STEPS} steps: {s}")
        assert s["num_clipped"] == STEPS and s["num_nonfinite"] == 0 and s["coef"] < 1.0 and s["total_norm"] >= 4e-3
    assert tg.optimizer._clip.stats() == te.optimizer._clip.stats()
    assert len(tg.losses) == STEPS and tg.losses == te.losses
    for a, b in zip(mg.parameters(), me.parameters()):
        assert torch.equal(a.detach(), b.detach())


def test_trainer_clipping_changes_the_run_and_a_huge_threshold_does_not(A, fits):
    (mc, tc), (mn, tn), (mh, th) = fits[(True, 1e-3)], fits[(True, None)], fits[(True, 1e9)]
    assert tn.optimizer._clip is None and tn.graphed.captures == 1 and th.graphed.captures == 1
    assert tc.losses[0] == tn.losses[0], "the first loss is computed before any update"
    assert tc.losses != tn.losses, (tc.losses, tn.losses)
    s = th.optimizer._clip.stats()
    assert s["num_clipped"] == 0 and s["coef"] == 1.0 and 0.0 < s["total_norm"] < 1e9
    assert th.losses == tn.losses
    for a, b in zip(mh.parameters(), mn.parameters()):
        assert torch.equal(a.detach(), b.detach())
