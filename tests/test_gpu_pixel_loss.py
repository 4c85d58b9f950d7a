"""The pixel losses on the MI355X (csrc/pixel_loss.hip through sr_amd.pixel_loss): the HIP loss and gradient of Charbonnier, Huber,
smooth-L1, the robust loss and the PSNR loss against the float64 statement of tests/pixel_loss_ref.py, determinism, the upstream
gradient, more images than a grid dimension and the most a launch takes, alphas at the edges of fp32, the PSNR metric, the torch
fallbacks, the refusals and the graphed training step."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_loss_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_IDS = [c[0] for c in REF.CASES]
ALL = [(cid, kind, params, shape) for cid, kind, params in REF.CASES for shape in REF.SHAPES] + \
      [("psnr", "psnr", {}, shape) for shape in REF.PSNR_SHAPES]
ALL_IDS = [f"{cid}-{'x'.join(map(str, shape))}" for cid, _, _, shape in ALL]
# one case per kernel instance, for the tests that run at one shape
KINDS = [c for c in REF.CASES if c[1] != "robust" or c[2]["c"] == 0.1] + [("psnr", "psnr", {})]
KIND_IDS = [c[0] for c in KINDS]


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


@functools.lru_cache(maxsize=None)
def _images(shape, psnr=False):
    return (REF.psnr_images if psnr else REF.images)(shape, 11 + sum(shape))


@functools.lru_cache(maxsize=None)
def _case(cid, shape):
    """(sr, hr, float64 loss, float64 gradient) of one case and shape: computed once, read by every test that needs it."""
    if cid == "psnr":
        sr, hr = _images(shape, True)
        return (sr, hr) + REF.loss_and_grad("psnr", sr, hr, {})
    _, kind, params = REF.CASES[CASE_IDS.index(cid)]
    sr, hr = _images(shape)
    return (sr, hr) + REF.loss_and_grad(kind, sr, hr, params)


def _apply(A, kind, params, s, h):
    """The HIP autograd functions themselves (no fallback decision)."""
    P = A.pixel_loss
    p = P.pixel_loss_check_params(kind, params)
    if kind == "psnr":
        return A.ops.PSNRLossFn.apply(s, h, p["eps"])
    return A.ops.PixelLossFn.apply(s, h, *P._kind_of(kind, p))


def _hip_loss_grad(A, kind, params, sr, hr, weight=None):
    s = sr.detach().cuda().float().contiguous().requires_grad_(True)
    loss = _apply(A, kind, params, s, hr.cuda().float().contiguous())
    # the upstream gradient arrives as a device scalar, the way a loss scaler hands it over
    (loss if weight is None else torch.tensor(weight, device="cuda") * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), s.grad.detach()


# The limits (REF.LIMITS, per loss: the loss's relative error, the gradient's relative L2, its max error over the largest entry) are
# ten times what the float64 statement itself costs when it runs in fp32 torch on these inputs (tests/test_pixel_loss_cpu.py measures
# that); the margin is for the kernel's summation order, sqrtf, division, expm1f and log1pf.  Nothing is excluded from a comparison.
@pytest.mark.parametrize("cid,kind,params,shape", ALL, ids=ALL_IDS)
def test_hip_matches_float64(A, cid, kind, params, shape):
    sr, hr, l64, g64 = _case(cid, shape)
    loss, g = _hip_loss_grad(A, kind, params, sr, hr)
    dl, l2, worst = REF.errors(loss, g, l64, g64)
    print(f"\n{cid} {shape}: loss {float(loss):.6g}, rel dloss {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and g.shape == sr.shape
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    assert dl <= REF.LIMIT_LOSS[kind]
    assert l2 <= REF.LIMIT_L2[kind]
    assert worst <= REF.LIMIT_MAX[kind]
    same = sr == hr
    if same.any():
        assert float(g.cpu()[same].abs().max()) == 0.0, "the gradient is exactly 0 where sr equals hr"
    if kind == "psnr" and shape[0] > 1:
        assert float(g[0].abs().max()) == 0.0 and float(g[1:].abs().max()) > 0.0, "the image equal to its target"


def test_psnr_more_images_than_a_grid_dimension(A):
    """65538 images: (image, block) share one grid dimension, so nothing wraps at 65535 and the last image gets its own gradient."""
    shape = (65538, 1, 2, 2)
    sr, hr, l64, g64 = _case("psnr", shape)
    _, g = _hip_loss_grad(A, "psnr", {}, sr, hr)
    assert float(g64[-1].abs().max()) > 0.0
    for n in (-1, 65535, 65536):
        err = (g[n].cpu().double() - g64[n]).abs().max() / g64[n].abs().max()
        assert float(err) <= REF.LIMIT_MAX["psnr"] * float(g64.abs().max() / g64[n].abs().max()), n


def test_psnr_most_images_a_launch_takes(A, monkeypatch):
    """2^24 - 1 images of one element: one block each, the largest grid below 2^32 threads, launches and is right to its last image;
    one image more is not launched and takes the torch path."""
    launched = []
    real = A._lib.call
    monkeypatch.setattr(A._lib, "call", lambda name, *a, **k: launched.append(name) or real(name, *a, **k))
    n = REF.PSNR_MOST_IMAGES
    sr, hr = REF.psnr_images((n + 1, 1, 1, 1), 9)
    l64, g64 = REF.loss_and_grad("psnr", sr[:n], hr[:n], {})
    s = sr[:n].cuda().requires_grad_(True)
    loss = A.ops.psnr_loss(s, hr[:n].cuda())
    loss.backward()
    assert launched == ["srk_psnr_loss_fwd", "srk_psnr_loss_finalize", "srk_psnr_loss_bwd"]
    dl, l2, worst = REF.errors(loss.detach(), s.grad, l64, g64)
    assert dl <= REF.LIMIT_LOSS["psnr"] and l2 <= REF.LIMIT_L2["psnr"] and worst <= REF.LIMIT_MAX["psnr"], (dl, l2, worst)
    tail = slice(n - 4096, n)
    assert float(g64[tail].abs().max()) > 0.0
    assert float((s.grad[tail].cpu().double() - g64[tail]).abs().max()) <= REF.LIMIT_MAX["psnr"] * float(g64.abs().max())
    del launched[:]
    more = float(A.ops.psnr_loss(sr.cuda(), hr.cuda()))
    assert launched == [] and abs(more - float(REF.psnr(sr.double(), hr.double()))) <= 1e-5 * abs(more)


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 16, 16)], ids=["1x3x5x7", "2x3x16x16"])
@pytest.mark.parametrize("alpha,kernel", REF.EDGE_ALPHAS, ids=[f"{a:g}" for a, _ in REF.EDGE_ALPHAS])
def test_robust_alphas_at_the_edges_of_fp32(A, monkeypatch, alpha, kernel, shape):
    """An alpha that fp32 rounds to 2, 0 or -inf runs that exact kernel, the smallest normal alpha the general one, a subnormal one
    none (float64 torch): all finite, all within the robust limits of the float64 statement at the alpha given."""
    kinds = []
    real = A._lib.call
    monkeypatch.setattr(A._lib, "call", lambda name, args, *a, **k: kinds.append(args.kind) or real(name, args, *a, **k))
    sr, hr = _images(shape)
    params = {"alpha": alpha, "c": 0.1}
    l64, g64 = REF.loss_and_grad("robust", sr, hr, params)
    s = sr.cuda().requires_grad_(True)
    loss = A.ops.robust_loss(s, hr.cuda(), **params)
    loss.backward()
    assert kinds == ([] if kernel is None else [getattr(A._lib, "SRK_PIXEL_" + kernel)] * 2)
    dl, l2, worst = REF.errors(loss.detach(), s.grad, l64, g64)
    print(f"\nalpha {alpha:g} {shape}: loss {float(loss.detach()):.6g}, rel dloss {dl:.2e}, grad rel L2 {l2:.2e}, max {worst:.2e}")
    assert loss.dtype == torch.float32 and torch.isfinite(loss) and torch.isfinite(s.grad).all()
    assert dl <= REF.LIMIT_LOSS["robust"] and l2 <= REF.LIMIT_L2["robust"] and worst <= REF.LIMIT_MAX["robust"]
    same = sr == hr
    assert same.any() and float(s.grad.cpu()[same].abs().max()) == 0.0


def test_psnr_loss_is_minus_the_psnr_metric(A):
    sr, hr = _images((2, 3, 16, 16), True)
    x, h = sr.clamp(0, 1).cuda(), hr.cuda()
    loss, metric = float(A.ops.psnr_loss(x, h)), float(A.ops.psnr(x, h))
    assert abs(loss + metric) <= REF.LIMIT_LOSS["psnr"] * abs(metric), (loss, metric)


@pytest.mark.parametrize("cid,kind,params", KINDS, ids=KIND_IDS)
def test_deterministic(A, cid, kind, params):
    sr, hr = _images((4, 3, 96, 81), kind == "psnr")
    l1, g1 = _hip_loss_grad(A, kind, params, sr, hr)
    l2, g2 = _hip_loss_grad(A, kind, params, sr, hr)
    assert float(l1) == float(l2) and torch.equal(g1, g2), "fixed-order reductions: bit-identical runs"


@pytest.mark.parametrize("cid,kind,params", KINDS, ids=KIND_IDS)
def test_upstream_gradient(A, cid, kind, params):
    shape = (3, 1, 33, 33) if kind == "psnr" else (2, 3, 16, 16)
    sr, hr, l64, g64 = _case(cid, shape)
    for weight in (3.5, 65536.0):
        loss, g = _hip_loss_grad(A, kind, params, sr, hr, weight)
        dl, l2, worst = REF.errors(loss, g, l64, weight * g64)
        assert dl <= REF.LIMIT_LOSS[kind] and l2 <= REF.LIMIT_L2[kind] and worst <= REF.LIMIT_MAX[kind], (weight, dl, l2, worst)


def test_fallbacks_take_the_torch_path(A, monkeypatch):
    """fp16 / bf16 inputs, a target that needs a gradient, shapes that only broadcast, and a contiguous view that starts one element
    into its storage take the torch path (the launcher is patched to raise) and agree with float64 on the values they hold."""
    P, L = A.pixel_loss, A._lib
    real = L.call

    def refuse(name, *a, **k):
        raise AssertionError(f"{name} launched")
    monkeypatch.setattr(L, "call", refuse)
    sr, hr = _images((2, 3, 16, 16))
    s, h = sr.cuda(), hr.cuda()
    buf_s, buf_h = torch.empty(s.numel() + 1, device="cuda"), torch.empty(s.numel() + 1, device="cuda")
    vs, vh = buf_s[1:].view(s.shape), buf_h[1:].view(s.shape)
    vs.copy_(s)
    vh.copy_(h)
    assert vs.is_contiguous() and vs.data_ptr() % 16 == 4
    entries = [("charbonnier", P.charbonnier_loss, {"eps": 1e-3}), ("huber", P.huber_loss, {"delta": 0.5}),
               ("smooth_l1", P.smooth_l1_loss, {"beta": 0.5}), ("robust", P.robust_loss, {"alpha": 0.5, "c": 0.1}),
               ("psnr", P.psnr_loss, {})]
    for kind, fn, params in entries:
        def check(a, b, ra, rb):
            """fn(a, b) with the gradient for a against the statement on the float64 values of (ra, rb)"""
            a = a.detach().requires_grad_(True)
            loss = fn(a, b, **params)
            loss.backward()
            l64, g64 = REF.loss_and_grad(kind, ra, rb.expand_as(ra), params)
            dl, l2, worst = REF.errors(loss.detach(), a.grad.float(), l64, g64)
            scale = 1.0 if a.dtype == torch.float32 else 2.0 ** (24 - (11 if a.dtype == torch.float16 else 8))   # the gradient's own rounding
            assert dl <= REF.LIMIT_LOSS[kind] and l2 <= scale * REF.LIMIT_L2[kind] and worst <= scale * REF.LIMIT_MAX[kind], (kind, a.dtype, dl, l2, worst)
        for dt in (torch.float16, torch.bfloat16):
            check(s.to(dt), h.to(dt), sr.to(dt), hr.to(dt))
        check(s, h.clone().requires_grad_(True), sr, hr)
        check(s, h[:1], sr, hr[:1])
        check(vs, vh, sr, hr)
        check(s, vh, sr, hr)
    monkeypatch.setattr(L, "call", real)
    launched = []
    monkeypatch.setattr(L, "call", lambda name, *a, **k: launched.append(name) or real(name, *a, **k))
    for kind, fn, params in entries:
        fn(s, h, **params)
    assert launched == ["srk_pixel_loss_fwd"] * 4 + ["srk_psnr_loss_fwd", "srk_psnr_loss_finalize"]


def test_refusals_of_the_c_entries(A):
    L = A._lib
    lib = L.load()
    x = torch.rand(64, device="cuda")
    y = torch.rand(64, device="cuda")
    part = torch.zeros(8, dtype=torch.float64, device="cuda")
    one = torch.ones((), device="cuda")
    grad = torch.zeros(64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def pixel(**over):
        f = dict(sr=x.data_ptr(), hr=y.data_ptr(), n=64, kind=L.SRK_PIXEL_CHARBONNIER, p0=1e-3, p1=0.0, partial=part.data_ptr(),
                 gout=one.data_ptr(), scale=1.0 / 64, grad=grad.data_ptr())
        return L.PixelLossArgs(**dict(f, **over))
    for name in ("srk_pixel_loss_fwd", "srk_pixel_loss_bwd"):
        for over in (dict(sr=0), dict(hr=0), dict(n=0), dict(kind=7), dict(kind=-1), dict(sr=x.data_ptr() + 4)):
            with pytest.raises(RuntimeError, match=name):
                L.call(name, pixel(**over), stream)
    with pytest.raises(RuntimeError):
        L.call("srk_pixel_loss_fwd", pixel(partial=0), stream)
    for over in (dict(gout=0), dict(grad=0), dict(grad=grad.data_ptr() + 4)):
        with pytest.raises(RuntimeError):
            L.call("srk_pixel_loss_bwd", pixel(**over), stream)
    coef = torch.zeros(2, device="cuda")
    out = torch.zeros((), device="cuda")

    def psnr(**over):
        f = dict(sr=x.data_ptr(), hr=y.data_ptr(), N=2, per=32, eps=1e-8, partial=part.data_ptr(), coef=coef.data_ptr(),
                 loss=out.data_ptr(), gout=one.data_ptr(), grad=grad.data_ptr())
        return L.PsnrLossArgs(**dict(f, **over))
    for name, overs in (("srk_psnr_loss_fwd", (dict(sr=0), dict(per=0), dict(partial=0), dict(hr=y.data_ptr() + 4))),
                        ("srk_psnr_loss_finalize", (dict(coef=0), dict(loss=0), dict(per=0), dict(eps=0.0))),
                        ("srk_psnr_loss_bwd", (dict(gout=0), dict(grad=0), dict(per=0), dict(coef=0)))):
        for over in overs:
            with pytest.raises(RuntimeError, match=name):
                L.call(name, psnr(**over), stream)
        import ctypes
        assert getattr(lib, name)(ctypes.byref(psnr(N=0)), ctypes.c_void_p(stream)) != 0, "no images"
    torch.cuda.synchronize()
    assert float(part.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0, "refused before any launch"


def _fit(A, use_graph, losses, loss_params):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.EDSR(scale_factor=2, precision=32, n_feats=32, n_resblocks=2, res_scale=0.1, losses=losses, loss_params=loss_params)
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 400 + i, "cpu") for i in range(8)))
    torch.cuda.synchronize()
    return tr, [p.detach().clone() for p in m.parameters()]


@pytest.mark.parametrize("losses,loss_params", [("0.5*l1+0.5*charbonnier", []), ("psnr", [])],
                         ids=["l1+charbonnier", "psnr"])
def test_graphed_step_follows_the_eager_loop(A, monkeypatch, losses, loss_params):
    launched = []
    real = A._lib.call
    monkeypatch.setattr(A._lib, "call", lambda name, *a, **k: launched.append(name) or real(name, *a, **k))
    family = "srk_psnr_loss_" if losses == "psnr" else "srk_pixel_loss_"
    tg, pg = _fit(A, True, losses, loss_params)
    captured = [n for n in launched if n.startswith(family)]
    assert family + "fwd" in captured and family + "bwd" in captured, "the captured step holds the HIP launches, not the torch path"
    del launched[:]
    te, pe = _fit(A, False, losses, loss_params)
    assert launched.count(family + "fwd") == launched.count(family + "bwd") == 8, "every eager step launched the HIP loss"
    g = tg.graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step with the pixel loss was captured"
    lg, le = tg.losses, te.losses
    assert len(lg) == len(le) == 8 and all(np.isfinite(lg))
    # every launch of the step sums in a fixed order ("Reproducibility"): the replayed step gives the eager loop's bits
    assert np.array_equal(np.asarray(lg, np.float32).view(np.int32), np.asarray(le, np.float32).view(np.int32)), (lg, le)
    diffs = [float((a - b).abs().max()) for a, b in zip(pg, pe)]
    print(f"\n{losses}: largest parameter difference {max(diffs):.2e} (tensor {diffs.index(max(diffs))} of {len(diffs)})")
    for a, b in zip(pg, pe):
        assert torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), diffs
