"""The kernels of the bench training step (EDSR-baseline x4, batch = one image per CU, 48x48 LR patches) in the launch geometry
that step runs them in, against float64.

At that batch the persistent launchers size their grids from `srk_device_cus()` and every workgroup walks several tiles, units
or images in turn (`tq` / `trem` split, halo prefetch of the next tile, several trunk images per CU).  The rest of the suite
mostly runs batches of 1-17, where each workgroup gets at most one tile.  Every case here is sized from the CU count, runs in
bf16 and fp16, asserts its geometry premise from the launcher's own formula before it checks numbers, and compares with a
float64 reference computed from the same 16-bit operands:

- per-image outputs (forward, data gradients) on >= 16 images: the first and the last, the images holding the first tile of
  the slots `trem - 1` and `trem`, and seeded others; these references run on the CPU;
- reductions (weight / bias gradients, the L1 sum) over the whole batch, chunked by image.  The full-batch convolution
  references are too large for the CPU in this module's time budget (the HR stage alone is about 1.5 TFLOP), so they run in
  float64 on the GPU through torch's own convolution (never an srk kernel).

Operands are integers times a power of two with at most 7 significant bits: exact in bf16 and in fp16, so that one float64
reference serves both types.  Outputs the test allocates are prefilled with NaN, so a tile that is never written shows up."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collapse_ref as R  # noqa: E402
from geometry_ref import (_check16, _check32, _eps, _ex, _geom, _nchw, _nhwc, _pick, _relerr,  # noqa: E402
                          _ws_premise)

pytestmark = pytest.mark.gpu
DT = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
CHUNK = 16          # images per float64 chunk of a full-batch reference (<= about 1 GB per float64 tensor at 96x96x256)


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


@pytest.fixture(scope="module")
def cus(A):
    c = int(A._lib.load().srk_device_cus())
    assert c > 0
    return c


@pytest.fixture(scope="module")
def cache():
    return {}


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the weight-stationary 3x3 64 -> 64 conv (the per-layer trunk path, conv_ws_kernel): forward epilogues and the masked dgrad
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", ["bench", "ragged"])
@pytest.mark.parametrize("variant", ["relu", "res_scale", "dgrad_mask"])
def test_ws_conv_multi_tile_walk(A, cus, dt, geom, variant):
    n, h, w = _geom(cus, geom)
    tiles_img, ntiles, slots = _ws_premise(cus, n, h, w, 64)
    if geom == "ragged":
        assert ntiles % slots != 0, "premise: the ragged shape has a remainder"
    g = torch.Generator().manual_seed(11 + len(variant) + n)
    x = _ex((n, h, w, 64), g, 7)
    wt = _ex((64, 64, 3, 3), g, 12)
    b = _ex((64,), g, 9)
    dev = torch.device("cuda")
    xd = x.to(dt).to(dev)
    out = torch.full((n, h, w, 64), float("nan"), dtype=dt, device=dev)
    res = mask = None
    if variant == "dgrad_mask":
        # ConvChainFn.backward of the first conv's output: dgrad through the transposed weights, * scale, ReLU mask of the activation
        act = torch.relu(_ex((n, h, w, 64), g, 7))
        mask = act.to(dt).to(dev)
        pk = A.ops.pack_conv(torch.nn.Parameter(wt.float().to(dev)), None, dt, dgrad=True)
        A.ops.conv_raw(xd, pk, N=n, H=h, W=w, Cin=64, Cout=64, out=out, scale=0.1, mask=mask, use_bias=False)
    else:
        if variant == "res_scale":
            res = _ex((n, h, w, 64), g, 7).to(dt).to(dev)
        pk = A.ops.pack_conv(torch.nn.Parameter(wt.float().to(dev)), torch.nn.Parameter(b.float().to(dev)), dt)
        A.ops.conv_raw(xd, pk, N=n, H=h, W=w, Cin=64, Cout=64, out=out, relu=variant == "relu",
                       scale=0.1 if res is not None else 1.0, res=res)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "an output tile was never written"
    imgs = _pick(n, tiles_img, ntiles, slots, seed=n)
    xs = _nchw(x[imgs])
    if variant == "dgrad_mask":
        ref = _nhwc(F.conv_transpose2d(xs, wt, padding=1)) * 0.1
        keep = act[imgs] > 0
        ref = torch.where(keep, ref, torch.zeros_like(ref))
        got = out[imgs].cpu()
        assert bool((got[~keep] == 0).all()), "masked elements are exactly zero"
    else:
        ref = _nhwc(F.conv2d(xs, wt, b, padding=1))
        if variant == "relu":
            ref = ref.clamp_min(0)
        else:
            ref = ref * 0.1 + res[imgs].double().cpu()
        got = out[imgs].cpu()
        if variant == "relu":
            assert bool((got[ref == 0] == 0).all()), "ReLU-zeroed elements are exactly zero"
    _check16(got, ref, dt, f"{variant} {geom} images {imgs}")


# ------------------------------------------------------------------------------------------------------------------------------
# 2. upsampler stage 1: 3x3 64 -> 256 + PixelShuffle store (ctiles = 4), its dgrad through the shuffle (conv_ks), its weight
#    gradient with dy_ps = 2 in the grouped ring
# ------------------------------------------------------------------------------------------------------------------------------
def _up_operands(n, h, w):
    g = torch.Generator().manual_seed(n * 7 + h)
    x = _ex((n, h, w, 64), g, 7)
    wt = _ex((256, 64, 3, 3), g, 12)
    b = _ex((256,), g, 9)
    gy = _ex((n, 2 * h, 2 * w, 64), g, 7)
    return x, wt, b, gy


def _up_wgrad_ref(x, gy, cache, key):
    """Full-batch float64 weight / bias gradient of conv(x) -> PixelShuffle(2) for upstream gy (GPU float64, torch's conv)."""
    if key not in cache:
        dev = torch.device("cuda")
        dw = torch.zeros(256, 64, 3, 3, dtype=torch.float64, device=dev)
        db = torch.zeros(256, dtype=torch.float64, device=dev)
        for n0 in range(0, x.shape[0], CHUNK):
            xc = _nchw(x[n0:n0 + CHUNK]).to(dev)
            gc = F.pixel_unshuffle(_nchw(gy[n0:n0 + CHUNK]).to(dev), 2)
            dw += torch.nn.grad.conv2d_weight(xc, (256, 64, 3, 3), gc, padding=1)
            db += gc.sum((0, 2, 3))
        cache[key] = (dw.cpu(), db.cpu())
    return cache[key]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", ["bench", "ragged"])
def test_upsampler_stage1_forward_dgrad_wgrad(A, cus, cache, dt, geom):
    n, h, w = _geom(cus, geom)
    dev = torch.device("cuda")
    tiles_img, ntiles, slots = _ws_premise(cus, n, h, w, 256)         # 64 slots per channel tile on 256 CUs
    ks_blocks = min(ntiles, cus)                                       # conv_ks: ncob = 1, one workgroup per CU
    assert ntiles // ks_blocks >= 2, "premise: conv_ks workgroups walk several tiles"
    th = 8 if n * tiles_img >= 1024 else 16
    assert th == 8, "premise: the grouped wgrad runs the 8-row ring"
    x, wt, b, gy = _up_operands(n, h, w)
    xd, gyd = x.to(dt).to(dev), gy.to(dt).to(dev)
    wp, bp = torch.nn.Parameter(wt.float().to(dev)), torch.nn.Parameter(b.float().to(dev))
    # forward: what ConvFn.forward launches for ps_r = 2
    out = torch.full((n, 2 * h, 2 * w, 64), float("nan"), dtype=dt, device=dev)
    pk = A.ops.pack_conv(wp, bp, dt, ps_r=2)
    A.ops.conv_raw(xd, pk, N=n, H=h, W=w, Cin=64, Cout=256, out=out, out_mode=A._lib.OUT_NHWC_PS, ps_r=2)
    # data gradient: what ConvFn.backward launches (reads dy through the shuffle addressing)
    gx = torch.full((n, h, w, 64), float("nan"), dtype=dt, device=dev)
    pkd = A.ops.pack_conv(wp, None, dt, dgrad=True, ps_r=2)
    A.ops.conv_raw(gyd, pkd, N=n, H=h, W=w, Cin=256, Cout=64, out=gx, x_ps=2, use_bias=False)
    # weight gradient: queued, then one grouped launch
    with A.ops.hold_wgrads():
        gw, gb = A.ops.wgrad(xd, gyd, wparam=wp, bparam=bp, N=n, H=h, W=w, Cin=64, Cout=256, k=3, w_shape=(256, 64, 3, 3), ps_r=2,
                             scale=1.0, dy_ps=2, want_bias=True)
        assert len(A.ops._WQ.jobs) == 1, "premise: the weight gradient is a grouped-ring job"
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all()), "an output tile was never written"
    imgs = _pick(n, tiles_img, ntiles, slots, seed=n + 1)
    xs = _nchw(x[imgs])
    ref = _nhwc(F.pixel_shuffle(F.conv2d(xs, wt, b, padding=1), 2))
    _check16(out[imgs].cpu(), ref, dt, f"stage-1 forward {geom}")
    imgs_k = _pick(n, -(-h // 16) * -(-w // 16), ntiles, ks_blocks, seed=n + 2)
    refx = _nhwc(F.conv_transpose2d(F.pixel_unshuffle(_nchw(gy[imgs_k]), 2), wt, padding=1))
    _check16(gx[imgs_k].cpu(), refx, dt, f"stage-1 dgrad {geom}")
    rw, rb = _up_wgrad_ref(x, gy, cache, ("up", geom))
    _check32(gw, rw, f"stage-1 dW {geom}")
    _check32(gb, rb, f"stage-1 db {geom}")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the collapsed HR stage (ops.hr_tail): lk5_rows_fwd / lk5_dgrad / lk5_wgrad and the edge kernels at split 1
# ------------------------------------------------------------------------------------------------------------------------------
_POST = (0.4488, 0.4371, 0.4040)


def _hr_operands(n, h, w):
    g = torch.Generator().manual_seed(n * 3 + w)
    x = _ex((n, h, w, 64), g, 7)
    wu = _ex((256, 64, 3, 3), g, 12)
    bu = _ex((256,), g, 9)
    wt = _ex((3, 64, 3, 3), g, 10)
    bt = _ex((3,), g, 8)
    gy = _ex((n, 3, 2 * h, 2 * w), g, 7)
    return x, wu, bu, wt, bt, gy


def _hr_wgrad_ref(x, wu, bu, wt, bt, gy, cache, key):
    """Full-batch float64 gradients of the two-layer form for the four parameters (GPU float64, torch's conv)."""
    if key not in cache:
        dev = torch.device("cuda")
        P = [t.to(dev).requires_grad_(True) for t in (wu, bu, wt, bt)]
        for n0 in range(0, x.shape[0], CHUNK):
            xc = _nchw(x[n0:n0 + CHUNK]).to(dev)
            y = R.layerwise(xc, P[2], P[3], P[0], P[1])
            y.backward(gy[n0:n0 + CHUNK].to(dev))
        cache[key] = [p.grad.cpu() for p in P]
    return cache[key]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", ["bench", "ragged"])
def test_hr_stage_forward_backward(A, cus, cache, dt, geom):
    n, h, w = _geom(cus, geom, hr=True)
    dev = torch.device("cuda")
    x, wu, bu, wt, bt, gy = _hr_operands(n, h, w)
    xd = x.to(dt).to(dev).requires_grad_(True)
    P = [t.float().to(dev).requires_grad_(True) for t in (wu, bu, wt, bt)]
    assert A.ops.hr_tail_ok(xd, P[0], P[2], 2), "premise: the collapsed path takes this shape"
    # lk5_rows_fwd_launch / lk5_dgrad: segs = cus / (N nb) -> 1, units = N nb > cus: every workgroup walks several units
    nb = (w + 27) // 28
    segs = max(min(cus // (n * nb), (h + 7) // 8), 1)
    assert segs == 1 and n * nb >= 2 * cus, f"premise: {n * nb} units over {cus} workgroups, {segs} segments"
    if geom == "ragged":
        assert (n * nb) % cus != 0
    # edge kernels: edge_split(N) == 1
    assert min(max((512 + 2 * n - 1) // (2 * n), 1), 8) == 1
    # lk5_wgrad: fewer slabs than 16x16 tiles
    a = A._lib.WgradArgs(x=xd.data_ptr(), x_pitch=64, x_coff=0, x_ps=0, dy=xd.data_ptr(), dy_pitch=16, dy_coff=0, dy_ps=0,
                         N=n, H=h, W=w, Cin=64, Cout=16, KH=5, KW=5, dwp=0, dbp=0, nslabs=0, dtype=A.ops._DT[dt], cout_real=0)
    slabs = int(A._lib.load().srk_wgrad_slabs(a))
    ntiles5 = n * -(-h // 16) * -(-w // 16)
    assert 0 < slabs and ntiles5 // slabs >= 2, f"premise: {ntiles5} tiles over {slabs} slabs"
    y = A.ops.hr_tail(xd, P[0], P[1], P[2], P[3], post_add=torch.tensor(_POST, device=dev))
    y.backward(gy.float().to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xd.grad).all())
    imgs = _pick(n, nb, n * nb, cus, seed=n + 3)
    X = _nchw(x[imgs]).clone().requires_grad_(True)
    ref = R.layerwise(X, wt, bt, wu, bu) + torch.tensor(_POST, dtype=torch.float64).view(1, 3, 1, 1)
    ref.backward(gy[imgs])
    tol = 6e-3 if dt == torch.bfloat16 else 1.2e-3                     # the collapsed weights are rounded to the compute type
    got = y[imgs].cpu().double()
    for i, im in enumerate(imgs):
        assert _relerr(got[i], ref[i]) < tol, f"forward image {im}"
    err = (got - ref.detach()).abs()
    assert float(err.max()) < 4 * tol * float(ref.detach().abs().max()), f"forward max err {float(err.max()):.3e}"
    gxr = _nhwc(X.grad)
    gxg = xd.grad[imgs].cpu().double()
    tolx = 2e-2 if dt == torch.bfloat16 else 3e-3
    for i, im in enumerate(imgs):
        assert _relerr(gxg[i], gxr[i]) < tolx, f"dx image {im}"
    assert float((gxg - gxr).abs().max()) < 4 * tolx * float(gxr.abs().max())
    # the parameter gradients: r = corr(x, g) from exact operands, expanded in fp32
    refs = _hr_wgrad_ref(x, wu, bu, wt, bt, gy, cache, ("hr", geom))
    for p, r, name in zip(P, refs, ("wu", "bu", "wt", "bt")):
        _check32(p.grad, r, f"HR stage d{name} {geom}", rel=1e-4, elem=2e-4)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the trunk launch (ops.res_trunk -> conv_trunk_kernel), forward and data-gradient tables, every layer checked on its own
#    16-bit input; two of the grouped weight gradients over the full batch
# ------------------------------------------------------------------------------------------------------------------------------
NB = 16


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("rounds", [1, 2], ids=["N=cus", "N=2cus"])
def test_trunk_every_layer(A, cus, cache, dt, rounds, monkeypatch):
    n, h, w = rounds * cus, 48, 48
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5 + rounds)
    x = _ex((n, h, w, 64), g, 7)
    W = [_ex((64, 64, 3, 3), g, 12) for _ in range(2 * NB + 1)]
    B = [_ex((64,), g, 9) for _ in range(2 * NB + 1)]
    gy = _ex((n, h, w, 64), g, 7)
    Wp = [torch.nn.Parameter(t.float().to(dev)) for t in W]
    Bp = [torch.nn.Parameter(t.float().to(dev)) for t in B]
    blocks = [((Wp[2 * b], Bp[2 * b]), (Wp[2 * b + 1], Bp[2 * b + 1])) for b in range(NB)]
    xd = x.to(dt).to(dev).requires_grad_(True)
    assert A.ops.res_trunk_ok(xd, blocks, (Wp[-1], Bp[-1])), "premise: the trunk launch takes this batch"
    assert n // cus == rounds and -(-h // 16) * -(-w // 16) == 9, "premise: 9 tiles per image, `rounds` images per CU"
    jobs = []
    real = A.ops.wgrad
    monkeypatch.setattr(A.ops, "wgrad", lambda a_in, dy, **kw: (jobs.append((a_in, dy, kw.get("scale", 1.0), kw["wparam"])), real(a_in, dy, **kw))[1])
    y = A.ops.res_trunk(xd, blocks, (Wp[-1], Bp[-1]), scale=0.1)
    sv = y.grad_fn.saved_tensors
    xs, hs = sv[:NB + 1], sv[NB + 1:2 * NB + 1]
    y.backward(gy.to(dt).to(dev))
    torch.cuda.synchronize()
    assert len(jobs) == 2 * NB + 1
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xd.grad).all())
    imgs = _pick(n, 9, n, cus, seed=rounds)
    imgs = sorted(set(imgs) | {cus - 1, n - 1} | ({cus} if rounds > 1 else set()))
    c = lambda t: _nchw(t[imgs].cpu().double())                      # noqa: E731
    conv = lambda t, i, bias=True: _nhwc(F.conv2d(c(t), W[i], B[i] if bias else None, padding=1))                   # noqa: E731
    convT = lambda t, i: _nhwc(F.conv_transpose2d(c(t), W[i], padding=1))                                          # noqa: E731
    # forward: every layer from the GPU's own 16-bit input
    for b in range(NB):
        ref = conv(xs[b], 2 * b).clamp_min(0)
        got = hs[b][imgs].cpu()
        assert bool((got[ref == 0] == 0).all()), f"block {b}: ReLU-zeroed elements are exactly zero"
        _check16(got, ref, dt, f"trunk fwd block {b} conv 1")
        ref = conv(hs[b], 2 * b + 1) * 0.1 + _nhwc(c(xs[b]))
        _check16(xs[b + 1][imgs].cpu(), ref, dt, f"trunk fwd block {b} conv 2")
    _check16(y[imgs].detach().cpu(), conv(xs[NB], 2 * NB) + x[imgs], dt, "trunk fwd tail conv")
    # backward: the data gradients are the dy of the weight-gradient jobs (ResTrunkFn.backward's order)
    dys = {id(p): (a_in, dy, sc) for a_in, dy, sc, p in jobs}
    gxs = {b + 1: dys[id(Wp[2 * b + 1])][1] for b in range(NB)}
    ghs = {b: dys[id(Wp[2 * b])][1] for b in range(NB)}
    gyd = gy.to(dt)
    _check16(gxs[NB][imgs].cpu(), convT(gyd, 2 * NB), dt, "trunk bwd tail conv")
    for b in range(NB - 1, -1, -1):
        keep = hs[b][imgs].cpu() > 0
        ref = torch.where(keep, convT(gxs[b + 1], 2 * b + 1) * 0.1, torch.zeros(()).double())
        got = ghs[b][imgs].cpu()
        assert bool((got[~keep] == 0).all()), f"block {b}: masked gradient elements are exactly zero"
        _check16(got, ref, dt, f"trunk bwd block {b} conv 2")
        if b > 0:
            _check16(gxs[b][imgs].cpu(), convT(ghs[b], 2 * b) + _nhwc(c(gxs[b + 1])), dt, f"trunk bwd block {b} conv 1")
    # the input gradient: block 0's conv 1 (stored) + the long skip's add, two roundings
    part = convT(ghs[0], 0) + _nhwc(c(gxs[1]))
    ref = part + gyd[imgs].double()
    got = xd.grad[imgs].cpu().double()
    eps = _eps(dt)
    tol = eps * 1.5 * (ref.abs() + part.abs()) + 4e-3 * eps + 1e-3 * float(ref.abs().max()) * (1 if dt == torch.bfloat16 else 0.1)
    assert bool(((got - ref).abs() <= tol).all()), f"trunk input gradient: max err {float((got - ref).abs().max()):.3e}"
    # weight gradients of the tail conv and of the last block's second conv (scale 0.1), full batch, GPU float64
    for i in (2 * NB, 2 * NB - 1):
        a_in, dy, sc = dys[id(Wp[i])]
        rw = torch.zeros(64, 64, 3, 3, dtype=torch.float64, device=dev)
        rb = torch.zeros(64, dtype=torch.float64, device=dev)
        for n0 in range(0, n, CHUNK):
            ac, dc = _nchw(a_in[n0:n0 + CHUNK].double()), _nchw(dy[n0:n0 + CHUNK].double())
            rw += torch.nn.grad.conv2d_weight(ac, (64, 64, 3, 3), dc, padding=1)
            rb += dc.sum((0, 2, 3))
        _check32(Wp[i].grad, rw * sc, f"trunk dW layer {i}")
        _check32(Bp[i].grad, rb * sc, f"trunk db layer {i}")


# ------------------------------------------------------------------------------------------------------------------------------
# 5. head: srk_unfold_nchw + the 1x1 conv over 27 (-> 32) unfolded channels, and its weight gradient (wgrad1x1_small_kernel)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", ["bench", "ragged"])
def test_head_conv_forward_wgrad(A, cus, dt, geom):
    n, h, w = _geom(cus, geom)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(n + 17)
    img = _ex((n, 3, h, w), g, 7, lo=0)
    sub = torch.tensor([-0.4488, -0.4371, -0.4040], dtype=torch.float64)
    wt = _ex((64, 3, 3, 3), g, 9)
    b = _ex((64,), g, 9)
    gy = _ex((n, h, w, 64), g, 7)
    tiles_img = -(-h // 16) * -(-w // 16)
    assert n * tiles_img >= 2 * cus, "premise: more than two 16x16 tiles per CU"
    wp, bp = torch.nn.Parameter(wt.float().to(dev)), torch.nn.Parameter(b.float().to(dev))
    # the 1x1 weight gradient runs in slab mode over fewer slabs than 64-pixel K tiles
    xu = A.ops.unfold_raw(img.float().to(dev), sub.float().to(dev), 3, dt)
    a = A._lib.WgradArgs(x=xu.data_ptr(), x_pitch=32, x_coff=0, x_ps=0, dy=xu.data_ptr(), dy_pitch=64, dy_coff=0, dy_ps=0,
                         N=n, H=h, W=w, Cin=32, Cout=64, KH=1, KW=1, dwp=0, dbp=0, nslabs=0, dtype=A.ops._DT[dt], cout_real=64)
    slabs = int(A._lib.load().srk_wgrad_slabs(a))
    assert 0 < slabs and (n * h * w // 64) // slabs >= 2, f"premise: {slabs} slabs"
    y = A.ops.head_conv(img.float().to(dev), wp, bp, sub.float().to(dev), dt)
    y.backward(gy.to(dt).to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    imgs = _pick(n, tiles_img, n * tiles_img, cus, seed=n + 4)
    # the unfolded operand: (x - sub) rounded once to the storage type, zero outside the image and in the 5 padding channels
    xs = img[imgs] - sub.view(1, 3, 1, 1)
    ref_u = F.unfold(xs, 3, padding=1).view(len(imgs), 27, h, w).permute(0, 2, 3, 1)
    gu = xu[imgs].cpu().double()
    assert bool((gu[..., 27:] == 0).all())
    _check16(gu[..., :27], ref_u, dt, "unfold")
    # forward from the GPU's own rounded operand
    ref = gu[..., :27].reshape(-1, 27) @ wt.reshape(64, 27).t() + b
    _check16(y[imgs].detach().cpu().reshape(-1, 64), ref, dt, f"head fwd {geom}")
    # weight gradient over the full batch (exact 16-bit products, fp32 accumulation)
    xa = xu.double()[..., :27].reshape(-1, 27)
    da = gy.to(dev).double().reshape(-1, 64)
    rw = (da.t() @ xa).reshape(64, 3, 3, 3).cpu()
    rb = da.sum(0).cpu()
    _check32(wp.grad, rw, f"head dW {geom}")
    _check32(bp.grad, rb, f"head db {geom}")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the L1 loss at the bench step's HR batch
# ------------------------------------------------------------------------------------------------------------------------------
def test_l1_loss_at_bench_batch(A, cus):
    dev = torch.device("cuda")
    shape = (cus, 3, 192, 192)
    nel = cus * 3 * 192 * 192
    nb = int(A._lib.load().srk_l1_blocks(nel))
    assert nel > 4 * 256 * nb * 2, f"premise: {nb} blocks each walk several 1024-element strides"
    g = torch.Generator().manual_seed(23)
    sr = torch.rand(shape, generator=g)
    hr = torch.rand(shape, generator=g)
    hr.view(-1)[::97] = sr.view(-1)[::97]                        # ties: sign 0, zero gradient
    srd = sr.to(dev).requires_grad_(True)
    loss = A.ops.l1_loss(srd, hr.to(dev))
    loss.backward(torch.tensor(3.0, device=dev))
    torch.cuda.synchronize()
    d = sr.double() - hr.double()
    ref = d.abs().mean()
    assert abs(float(loss) - float(ref)) <= 2e-7 * float(ref), (float(loss), float(ref))
    want = torch.sign(d).float() * (torch.tensor(1.0 / nel, dtype=torch.float32) * 3.0)
    got = srd.grad.cpu()
    assert bool((got[d == 0] == 0).all())
    assert float((got - want).abs().max()) <= 2 * float(want.abs().max()) * 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------------------------
# 7. one whole eager training step of the bench model at batch = cus, against float64 on a subset of images
# ------------------------------------------------------------------------------------------------------------------------------
KW = dict(n_feats=64, n_resblocks=16, res_scale=0.1)
PREC = {torch.bfloat16: "bf16", torch.float16: 16}


def _step_subset(cus):
    # first / last image, the images on either side of the round boundary, seeded others: 8 in all
    s = {0, cus - 1, cus // 2 - 1, cus // 2}
    g = torch.Generator().manual_seed(31)
    for i in torch.randperm(cus, generator=g).tolist():
        if len(s) >= 8:
            break
        s.add(i)
    return sorted(s)


@pytest.fixture(scope="module")
def step_ref(cus):
    """float64 CPU reference of the bench model on the subset S: the image and every parameter gradient of sum(y * t)."""
    from oracle import functional as OF
    import sr_amd
    torch.manual_seed(0)                                              # bench.py's model
    m = sr_amd.EDSR(scale_factor=4, precision=32, **KW)
    S = _step_subset(cus)
    g = torch.Generator().manual_seed(41)
    lr = torch.rand(cus, 3, 48, 48, generator=g)
    t = torch.zeros(cus, 3, 192, 192)
    t[S] = torch.rand(len(S), 3, 192, 192, generator=g) - 0.5
    sd = {k: v.detach().double().clone() for k, v in m.state_dict().items()}
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    for k in names:
        sd[k].requires_grad_(True)
    y = OF.forward("EDSR", sd, lr[S].double(), scale_factor=4, **KW)
    (y * t[S].double()).sum().backward()
    return dict(state=m.state_dict(), S=S, lr=lr, t=t, y=y.detach(), grads={k: sd[k].grad for k in names})


def _run_step(A, state, lr, t, dt):
    dev = torch.device("cuda")
    m = A.EDSR(scale_factor=4, precision=PREC[dt], **KW).to(dev)
    m.load_state_dict(state)
    launches = []
    real = A.ops._trunk_launch
    A.ops._trunk_launch = lambda layers, d: (launches.append(len(layers)), real(layers, d))[1]
    try:
        y = m(lr.to(dev))
        (y * t.to(dev)).sum().backward()
        torch.cuda.synchronize()
    finally:
        A.ops._trunk_launch = real
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.requires_grad}
    return y.detach().cpu(), grads, launches


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_whole_step_at_batch_cus(A, cus, step_ref, dt):
    """Batch = cus (the trunk launch, the multi-tile walks) against float64 on S, with the tolerance set by the same S run as a
    batch of |S| (conv_pair, at most one tile per workgroup: pinned against float64 elsewhere)."""
    S, lr, t = step_ref["S"], step_ref["lr"], step_ref["t"]
    y_big, g_big, l_big = _run_step(A, step_ref["state"], lr, t, dt)
    nl = 2 * KW["n_resblocks"] + 1
    assert l_big == [nl, nl + 1], f"premise: one trunk launch forward, one backward (+ the long skip's add): {l_big}"
    assert bool(torch.isfinite(y_big).all())
    y_small, g_small, l_small = _run_step(A, step_ref["state"], lr[S], t[S], dt)
    assert l_small == [], "the small batch takes the per-block path"
    rows = [("y", _relerr(y_big[S], step_ref["y"]), _relerr(y_small, step_ref["y"]))]
    for k, r in step_ref["grads"].items():
        rows.append((k, _relerr(g_big[k], r), _relerr(g_small[k], r)))
    print(f"\n[{DT_IDS[DT.index(dt)]}] relative error vs float64: batch {lr.shape[0]} / batch {len(S)}")
    for k, eb, es in rows:
        print(f"  {k:32s} {eb:.3e} {es:.3e}")
    bad = [(k, eb, es) for k, eb, es in rows if not eb <= 1.5 * es + 1e-6]
    assert not bad, f"batch-{lr.shape[0]} error above 1.5 x the batch-{len(S)} error: {bad}"
