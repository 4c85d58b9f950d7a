"""The frequency losses on the MI355X (csrc/freq_loss.hip through sr_amd.freq_loss): the HIP loss and gradient of `fft` and `ffl`
against the float64 statement of tests/freq_loss_ref.py, the upstream gradient, determinism, a captured and replayed forward and
backward, the routing to the torch path, and the training step."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import freq_loss_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ("fft", "ffl")
IDS = ["x".join(map(str, s)) for s in REF.SHAPES]


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


@functools.lru_cache(maxsize=None)
def _case(kind, shape, alpha=1.0):
    """(sr, hr, float64 loss, float64 gradient): computed once, read by every test that needs it."""
    sr, hr = REF.case(kind, shape)
    return (sr, hr) + REF.loss_and_grad(kind, sr, hr, alpha=alpha)


def _apply(A, kind, s, h, alpha=1.0):
    return A.ops.FFTLossFn.apply(s, h) if kind == "fft" else A.ops.FFLLossFn.apply(s, h, alpha)


def _hip_loss_grad(A, kind, sr, hr, weight=1.0, alpha=1.0):
    s = sr.detach().cuda().requires_grad_(True)
    loss = _apply(A, kind, s, hr.cuda(), alpha)
    (weight * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), s.grad.detach()


def _within(e, kind):
    return all(x <= lim for x, lim in zip(e, REF.LIMIT[kind]))


# The limits (REF.LIMIT: ten times the floors REF.FLOOR that the statement in fp32 costs against itself in float64) hold for every
# element: the inputs keep every non-structural component of D at least 5e-4 rms(D) from zero (tests/test_freq_loss_cpu.py), so no
# sign of D differs between fp32 and float64.  A workgroup owns 32 rows of the half spectrum (k = 0 .. H / 2) and a wave 32 columns:
# 1 x 1 and 2 x 2 are all structure; 5 x 7 and 33 x 31 have no Nyquist row; 32 x 32 is one MFMA tile and 17 spectrum rows; 37 x 71
# is ragged both ways with three waves; 192 x 192 has four row blocks (the last holds the Nyquist row alone) and six waves; 100 x 260
# nine waves and two row blocks.
@pytest.mark.parametrize("shape", REF.SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_hip_matches_float64(A, kind, shape):
    sr, hr, l64, g64 = _case(kind, shape)
    loss, g = _hip_loss_grad(A, kind, sr, hr)
    e = REF.errors(loss, g, l64, g64)
    print(f"\n{kind} {shape}: loss {float(loss):.6f}, |dloss|/loss {e[0]:.2e}, grad rel L2 {e[1]:.2e}, max {e[2]:.2e}")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and g.shape == sr.shape
    assert torch.isfinite(g).all()
    assert _within(e, kind), (e, REF.LIMIT[kind])
    if kind == "ffl" and shape[0] > 1:
        assert float(g[0].abs().max()) == 0.0, "the image equal to its target has q_max = 0 and gets no gradient"
        assert float(g[1:].abs().max()) > 0.0


@pytest.mark.parametrize("alpha", [0.0, 0.5, 3.0, 8.0])
def test_ffl_alphas(A, alpha):
    shape = (3, 3, 48, 40)
    sr, hr, l64, g64 = _case("ffl", shape, alpha)
    loss, g = _hip_loss_grad(A, "ffl", sr, hr, alpha=alpha)
    e = REF.errors(loss, g, l64, g64)
    print(f"\nalpha {alpha}: {e}")
    assert _within(e, "ffl"), (e, REF.LIMIT["ffl"])
    if alpha == 0.0:
        want = float(torch.nn.functional.mse_loss(sr.double(), hr.double()))
        assert abs(float(loss) - want) <= REF.LIMIT["ffl"][0] * want, "Parseval"


def test_one_pixel_and_identical_images(A):
    sr, hr = torch.tensor([[[[0.75]]]]), torch.tensor([[[[0.25]]]])
    loss, g = _hip_loss_grad(A, "fft", sr, hr)
    assert float(loss) == 0.25 and float(g) == 0.5
    z = torch.rand(2, 3, 40, 24)
    for kind in KINDS:
        loss, g = _hip_loss_grad(A, kind, z, z)
        assert float(loss) == 0.0 and float(g.abs().max()) == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_upstream_gradient(A, kind):
    """(0.3 * loss).backward() and a composite with l1: the backward reads the upstream gradient on the device."""
    sr, hr, l64, g64 = _case(kind, (3, 3, 48, 40))
    l1, g1 = _hip_loss_grad(A, kind, sr, hr)
    l3, g3 = _hip_loss_grad(A, kind, sr, hr, weight=0.3)
    assert float(l3) == float(l1) and float(g1.abs().max()) > 0.0
    assert torch.allclose(g3, 0.3 * g1, rtol=1e-6, atol=0.0)
    s, h = sr.cuda().requires_grad_(True), hr.cuda()
    fn = A.ops.fft_loss if kind == "fft" else A.ops.ffl_loss
    total = 0.95 * A.ops.l1_loss(s, h) + 0.05 * fn(s, h)
    total.backward()
    want = 0.95 * torch.sign(sr.double() - hr.double()) / sr.numel() + 0.05 * g64
    got = s.grad.cpu().double()
    assert float((got - want).norm() / want.norm()) <= REF.LIMIT[kind][1]


@pytest.mark.parametrize("kind", KINDS)
def test_deterministic(A, kind):
    sr, hr = REF.case(kind, (2, 3, 96, 81))
    l1, g1 = _hip_loss_grad(A, kind, sr, hr)
    l2, g2 = _hip_loss_grad(A, kind, sr, hr)
    assert float(l1) == float(l2) and torch.equal(g1, g2), "fixed-order reductions, no atomics: bit-identical runs"


@pytest.mark.parametrize("kind", KINDS)
def test_captured_forward_and_backward_replay(A, kind):
    """A straight-line graph of forward and backward, replayed after the input buffers were overwritten with a second image pair,
    gives what an eager run on that pair gives, bit for bit."""
    shape = (2, 3, 48, 40)
    (sr1, hr1), (sr2, hr2) = REF.case(kind, shape), (REF.images if kind == "fft" else REF.ffl_images)(shape, 99)
    want_l, want_g = _hip_loss_grad(A, kind, sr2, hr2)              # (eager first: it also builds the twiddle tables)
    s, h = sr1.cuda().requires_grad_(True), hr1.cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _apply(A, kind, s, h).backward()                            # warm-up on the side stream
        s.grad = None
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = _apply(A, kind, s, h)
        (grad,) = torch.autograd.grad(loss, s)
    with torch.no_grad():
        s.copy_(sr2.cuda())
        h.copy_(hr2.cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert float(loss.detach()) == float(want_l) and torch.equal(grad, want_g)
    assert not torch.equal(want_g, _hip_loss_grad(A, kind, sr1, hr1)[1]), "the two pairs differ"


@pytest.mark.parametrize("kind", KINDS)
def test_routing_to_the_torch_path(A, kind, monkeypatch):
    """fp16 / bf16 inputs, strided views, a 513-wide image and a target that needs a gradient compute in torch and agree with the
    statement: fp32 torch arithmetic keeps REF.LIMIT (the statement's own fp32 floor times ten); the 16-bit inputs are compared with
    the statement on the values they hold."""
    calls = []
    cls = A.ops.FFTLossFn if kind == "fft" else A.ops.FFLLossFn
    real = cls.apply
    monkeypatch.setattr(cls, "apply", lambda *a: calls.append(1) or real(*a))
    fn = A.ops.fft_loss if kind == "fft" else A.ops.ffl_loss
    sr, hr, l64, g64 = _case(kind, (3, 3, 48, 40))

    def check(s, h, ref=None):
        s = s.detach().requires_grad_(True)
        loss = fn(s, h)
        loss.backward()
        l, g = ref if ref is not None else (l64, g64)
        e = REF.errors(loss.detach().float(), s.grad.float(), l, g)
        assert _within(e, kind), (e, REF.LIMIT[kind])

    check(sr.cuda(), hr.cuda().requires_grad_(True))
    wide_s, wide_h = torch.zeros(3, 3, 48, 44, device="cuda"), torch.zeros(3, 3, 48, 44, device="cuda")
    wide_s[..., :40], wide_h[..., :40] = sr.cuda(), hr.cuda()
    assert not wide_s[..., :40].is_contiguous()
    check(wide_s[..., :40], wide_h[..., :40])
    check(sr.cuda(), wide_h[..., :40])
    for dt in (torch.float16, torch.bfloat16):
        s16, h16 = sr.to(dt), hr.to(dt)
        if kind == "ffl":
            s16[0] = h16[0]
        ref = REF.loss_and_grad(kind, s16.double(), h16.double())
        s = s16.cuda().requires_grad_(True)
        loss = fn(s, h16.cuda())
        loss.backward()
        e = REF.errors(loss.detach().float(), s.grad.float(), *ref)
        # the loss is fp32 arithmetic on the 16-bit values; the gradient comes back rounded to the input's format: half an ulp of
        # the largest entry (2^-11 / 2^-8 of it), and for fp16, whose subnormals are 2^-24 apart, at least 2^-25
        half_ulp = (2.0 ** -11, 2.0 ** -25) if dt == torch.float16 else (2.0 ** -8, 0.0)
        top = float(ref[1].abs().max())
        assert e[0] <= REF.LIMIT[kind][0] and e[2] * top <= (half_ulp[0] + REF.LIMIT[kind][2]) * top + half_ulp[1], e
    big_s, big_h = REF.case(kind, (1, 1, 6, 513))
    check(big_s.cuda(), big_h.cuda(), REF.loss_and_grad(kind, big_s, big_h))
    assert calls == []
    check(sr.cuda(), hr.cuda())
    assert calls == [1]
    if kind == "ffl":
        assert float(A.ops.ffl_loss(sr.cuda(), hr.cuda(), alpha=9.0)) > 0.0 and calls == [1], "alpha beyond 8 computes in torch"


def test_training_step_with_fft(A):
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision=32, n_feats=32, n_resblocks=2, res_scale=0.1, losses="0.95*l1+0.05*fft").cuda()
    g = torch.Generator().manual_seed(3)
    batch = {"lr": torch.rand(2, 3, 24, 24, generator=g).cuda(), "hr": torch.rand(2, 3, 48, 48, generator=g).cuda()}
    out = m.training_step(batch, 0)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert set(out) >= {"loss", "loss/l1", "loss/fft"} and torch.isfinite(out["loss"])
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
