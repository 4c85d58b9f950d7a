"""The kernels that only RCAN, RDN-B, WDSR-B, D-DBPN and SRResNet launch, in the geometry of their bench step (batch = one image
per CU, 48x48 LR patches), against float64.

bench.py runs every model at batch 256, where the persistent launchers size their grids from `srk_device_cus()` and every
workgroup walks many tiles, slabs, slices or pixel ranges; the rest of the suite runs batches of 1-17, where each gets one.  This
module follows test_gpu_step_geometry.py (the EDSR-baseline step): two geometries per case, 'bench' (N = cus at 48x48 LR,
192x192 HR) and 'ragged' (N = cus + 37 at 47x50, every walk with a nonzero remainder), both in bf16 and fp16.  Each case asserts
its geometry premise from the launcher (an exported helper, or the launcher's formula restated) before it checks numbers, so a
retune that makes the walk trivial fails here instead of passing silently.

Operands are integers times a power of two with at most 7 significant bits (exact in bf16 and fp16: one float64 reference
serves both types).  The full-batch operands are drawn on the GPU and kept in 16 bits there (a float64 host copy of the
SRResNet tail's input would be about 5 GB).  Outputs the test allocates, and the slab / slice scratch where the API takes the
caller's buffer, are prefilled with NaN, so a unit that is never written shows up.  Per-image outputs are compared on >= 16
images (the first and the last, the images holding the units on either side of the remainder, seeded others) against float64
on the CPU; reductions over the whole batch (weight / bias / slope gradients, BatchNorm statistics) against float64 on the GPU
through torch's own ops, chunked by image, never an srk kernel."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geometry_ref import _check16, _check32, _ex, _geom, _nchw, _nhwc, _pick  # noqa: E402

pytestmark = pytest.mark.gpu
DT = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
GEOMS = ["bench", "ragged"]
CHUNK = 16          # images per float64 chunk of a full-batch reference


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


def _exd(shape, seed, p, dt, lo=-127, hi=127):
    """_ex drawn on the GPU and stored in `dt`: the same integers for every dtype, so the float64 reference is shared."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = torch.randint(lo, hi + 1, tuple(shape), generator=g, device="cuda", dtype=torch.int16)
    return k.to(dt).mul_(2.0 ** -p)


def _nan(shape, dt):
    return torch.full(tuple(shape), float("nan"), dtype=dt, device="cuda")


def _pick_strided(n, tiles_img, ntiles, grid, seed):
    """Images for a walk `for (t = wg; t < ntiles; t += grid)`: those of _pick plus the images holding the last tile of the
    last full round, the first tile of the partial round and the last tile."""
    tq = ntiles // grid
    extra = {(tq * grid - 1) // tiles_img, min(tq * grid, ntiles - 1) // tiles_img, (ntiles - 1) // tiles_img}
    return sorted(set(_pick(n, tiles_img, ntiles, grid, seed=seed)) | extra)


def _cpu(t, imgs):
    return t[imgs].double().cpu()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. D-DBPN projections (csrc/proj.hip): srk_proj_up / srk_proj_down with and without the fused PReLU, srk_proj_wgrad + finalize
# ------------------------------------------------------------------------------------------------------------------------------
def _proj_premise(cus, n, lh, lw, geom):
    """proj_{up,down}_kernel: grid_for(nt) = min(nt, 2 cus) workgroups, each walks tiles wg, wg + grid, ... of 8x4 LR pixels."""
    tiles_img = -(-lw // 8) * -(-lh // 4)
    nt = n * tiles_img
    grid = min(nt, 2 * cus)
    assert nt // grid >= 2, f"premise: {nt} tiles over {grid} workgroups is not the multi-tile walk"
    if geom == "ragged":
        assert nt % grid != 0, "premise: the ragged shape has a remainder"
    return tiles_img, nt, grid


def _proj_weights(n):
    g = torch.Generator().manual_seed(900 + n)
    return _ex((32, 32, 8, 8), g, 12), _ex((32,), g, 9), _ex((32,), g, 7, lo=-32, hi=64)


def _proj_ref(x, wt, b, up, imgs, cache, key):
    if key not in cache:
        xs = _nchw(_cpu(x, imgs))
        y = F.conv_transpose2d(xs, wt, b, stride=4, padding=2) if up else F.conv2d(xs, wt, b, stride=4, padding=2)
        cache[key] = _nhwc(y)
    return cache[key]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
@pytest.mark.parametrize("act", ["none", "prelu1", "prelu32"])
def test_proj_forward_multi_tile_walk(A, cus, cache, dt, geom, up, act):
    L = A._lib
    n, lh, lw = _geom(cus, geom)
    tiles_img, nt, grid = _proj_premise(cus, n, lh, lw, geom)
    h, w = (lh, lw) if up else (4 * lh, 4 * lw)
    x = _exd((n, h, w, 32), 100 + n + up, 7, dt)
    wt, b, sl = _proj_weights(n)
    if act == "prelu1":
        sl = sl[:1]
    dev = torch.device("cuda")
    wpk = A.ops.proj_pack(wt.float().to(dev), dt, dev)
    half = L.load().srk_proj_pack_bytes() // 2
    bd = b.float().to(dev)
    sd = None if act == "none" else sl.float().to(dev)
    oshape = (n, 4 * lh, 4 * lw, 32) if up else (n, lh, lw, 32)
    out = _nan(oshape, dt)
    pre = None if sd is None else _nan(oshape, dt)
    L.call("srk_proj_up" if up else "srk_proj_down",
           L.ProjArgs(x=x.data_ptr(), x_pitch=32, out=out.data_ptr(), out_pitch=32, wpk=(wpk[half:] if up else wpk[:half]).data_ptr(),
                      bias=bd.data_ptr(), N=n, H=lh, W=lw, dtype=A.ops._DT[dt], slope=0 if sd is None else sd.data_ptr(),
                      slope_stride=0 if (sd is None or sd.numel() == 1) else 1, pre=0 if pre is None else pre.data_ptr(), pre_pitch=32),
           A.ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "an output tile was never written"
    imgs = _pick_strided(n, tiles_img, nt, grid, seed=n + up)
    ref = _proj_ref(x, wt, b, up, imgs, cache, ("proj", geom, up))
    what = f"proj {'up' if up else 'down'} {act} {geom} images {imgs}"
    if sd is None:
        _check16(_cpu(out, imgs), ref, dt, what)
        return
    assert bool(torch.isfinite(pre).all()), "a pre-activation tile was never written"
    _check16(_cpu(pre, imgs), ref, dt, what + " (pre)")
    # the activation is applied to the STORED conv output (one more rounding)
    p = _cpu(pre, imgs)
    a = sl.view(1, 1, 1, -1)
    _check16(_cpu(out, imgs), torch.where(p > 0, p, p * a), dt, what)


def _proj_wgrad_ref(xh, gl, cache, key):
    """Full-batch float64 dW [cl][ch][8][8] (conv2d(HR, W) = LR, either direction) and the two bias sums (GPU, torch's conv)."""
    if key not in cache:
        dw = torch.zeros(32, 32, 8, 8, dtype=torch.float64, device="cuda")
        for n0 in range(0, xh.shape[0], CHUNK):
            dw += torch.nn.grad.conv2d_weight(_nchw(xh[n0:n0 + CHUNK].double()), (32, 32, 8, 8), _nchw(gl[n0:n0 + CHUNK].double()),
                                              stride=4, padding=2)
        cache[key] = (dw.cpu(), gl.double().sum((0, 1, 2)).cpu(), xh.double().sum((0, 1, 2)).cpu())
    return cache[key]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("case", ["bias_lr", "bias_hr", "accumulate"])
def test_proj_wgrad_slices(A, cus, cache, dt, geom, case):
    L = A._lib
    n, lh, lw = _geom(cus, geom)
    ntw = n * -(-lw // 8) * -(-lh // 8)
    floats = int(L.load().srk_proj_wgrad_scratch_floats(n, lh, lw))
    ns = floats // (65536 + 8 * 32)
    assert ns * (65536 + 8 * 32) == floats
    assert ns == cus // 2 and ntw >= 16 * (cus // 2), f"premise: the cus/2-slice branch of wgrad_slices ({ntw} tiles, {ns} slices)"
    per = -(-ntw // ns)
    assert per >= 2, f"premise: {per} tiles per slice"
    if geom == "ragged":
        assert ntw % ns != 0, "premise: the ragged shape has a remainder"
    xh = _exd((n, 4 * lh, 4 * lw, 32), 200 + n, 7, dt)
    gl = _exd((n, lh, lw, 32), 300 + n, 7, dt)
    side = 1 if case == "bias_lr" else 2
    acc = int(case == "accumulate")
    scratch = _nan((floats,), torch.float32)
    g = torch.Generator().manual_seed(17)
    dw0, db0 = _ex((32, 32, 8, 8), g, 1), _ex((32,), g, 1)
    dw = dw0.float().cuda() if acc else _nan((32, 32, 8, 8), torch.float32)
    db = db0.float().cuda() if acc else _nan((32,), torch.float32)
    L.call("srk_proj_wgrad", L.ProjWgradArgs(xh=xh.data_ptr(), xh_pitch=32, g=gl.data_ptr(), g_pitch=32, scratch=scratch.data_ptr(),
                                             dw=dw.data_ptr(), accumulate=acc, N=n, H=lh, W=lw, dtype=A.ops._DT[dt], db=db.data_ptr(),
                                             bias_side=side, db_accumulate=acc), A.ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(scratch).all()), "a slice's partial was never written"
    rw, rb_lr, rb_hr = _proj_wgrad_ref(xh, gl, cache, ("projw", geom))
    rb = rb_lr if side == 1 else rb_hr
    if acc:
        rw, rb = rw + dw0, rb + db0
    _check32(dw, rw, f"proj dW {case} {geom}")
    _check32(db, rb, f"proj db {case} {geom}")


# ------------------------------------------------------------------------------------------------------------------------------
# 2. SRResNet's 9x9 tail conv 64 -> 3 at HR (csrc/conv_lk.hip): lk_conv_rows_kernel, the data gradient, the all-rows weight gradient
# ------------------------------------------------------------------------------------------------------------------------------
def _lk_refs(x, gy, wt, b, imgs, cache, key):
    if key not in cache:
        xs = _nchw(_cpu(x, imgs))
        y = _nhwc(F.conv2d(xs, wt, b, padding=4))
        gx = _nhwc(F.conv_transpose2d(_nchw(_cpu(gy, imgs)[..., :3]), wt, padding=4))
        dw = torch.zeros(3, 64, 9, 9, dtype=torch.float64, device="cuda")
        for n0 in range(0, x.shape[0], CHUNK):
            dw += torch.nn.grad.conv2d_weight(_nchw(x[n0:n0 + CHUNK].double()), (3, 64, 9, 9), _nchw(gy[n0:n0 + CHUNK, ..., :3].double()),
                                              padding=4)
        cache[key] = (y, gx, dw.cpu(), gy[..., :3].double().sum((0, 1, 2)).cpu())
    return cache[key]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", GEOMS)
def test_srresnet_tail_9x9(A, cus, cache, dt, geom):
    L = A._lib
    n, lh, lw = _geom(cus, geom)
    h, w = 4 * lh, 4 * lw
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(41)
    wt, b = _ex((3, 64, 9, 9), g, 12), _ex((3,), g, 9)
    x = _exd((n, h, w, 64), 400 + n, 7, dt).requires_grad_(True)
    gy = _exd((n, h, w, 16), 500 + n, 7, dt)
    gy[..., 3:] = 0
    # the forward takes lk_conv_rows_kernel (Cin 64, cout_real <= 4, cout_real * K <= 32, 16 stored channels) and the weight
    # gradient the all-rows kernel: cus slabs of 8x16 tiles, each walks tq (+1) of them
    assert 3 * 9 <= 32, "premise: cout_real * K <= 32 (lk_all_rows)"
    a = L.WgradArgs(x=x.data_ptr(), x_pitch=64, x_coff=0, x_ps=0, dy=gy.data_ptr(), dy_pitch=16, dy_coff=0, dy_ps=0, N=n, H=h, W=w,
                    Cin=64, Cout=16, KH=9, KW=9, dwp=0, dbp=0, nslabs=0, dtype=A.ops._DT[dt], cout_real=3)
    slabs = int(L.load().srk_wgrad_slabs(a))
    nt8 = n * -(-h // 8) * -(-w // 16)
    assert slabs == min(nt8, cus) == cus and nt8 // slabs >= 2, f"premise: {nt8} tiles over {slabs} slabs"
    if geom == "ragged":
        assert nt8 % slabs != 0, "premise: the ragged shape has a remainder"
    wp, bp = torch.nn.Parameter(wt.float().to(dev)), torch.nn.Parameter(b.float().to(dev))
    y = A.ops.conv_general(x, wp, bp, stride=1, pad=4)
    assert y.shape[3] == 16
    y.backward(gy)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all())
    imgs = _pick(n, -(-h // 8) * -(-w // 16), nt8, slabs, seed=n + 5)
    ry, rgx, rw, rb = _lk_refs(x.detach(), gy, wt, b, imgs, cache, ("lk", geom))
    got = _cpu(y.detach(), imgs)
    assert bool((got[..., 3:] == 0).all()), "padding channels are zeros"
    _check16(got[..., :3], ry, dt, f"9x9 tail forward {geom} images {imgs}")
    _check16(_cpu(x.grad, imgs), rgx, dt, f"9x9 tail dgrad {geom} images {imgs}")
    _check32(wp.grad, rw, f"9x9 tail dW {geom}")
    _check32(bp.grad, rb, f"9x9 tail db {geom}")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. SRResNet's BatchNorm + PReLU (ops.batch_norm_prelu: srk_chan_stats + the fused finalize, srk_chan_apply) at P = cus * 48 * 48
# ------------------------------------------------------------------------------------------------------------------------------
def _stats_premise(A, P, geom):
    nb = int(A._lib.load().srk_chan_stats_blocks(P))
    ppb = -(-P // nb)
    assert nb == 1024 and ppb >= 2 * 256, f"premise: the 1024-block cap, {ppb} pixels per block (several rounds of 256)"
    if geom == "ragged":
        assert P % nb != 0, "premise: the ragged shape has a remainder"
    return nb, ppb


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("npar", [1, 64])
def test_srresnet_batchnorm_prelu(A, cus, dt, geom, npar):
    n, h, w = _geom(cus, geom)
    _stats_premise(A, n * h * w, geom)
    dev = torch.device("cuda")
    x = _exd((n, h, w, 64), 600 + n, 5, dt).requires_grad_(True)
    gy = _exd((n, h, w, 64), 700 + n, 7, dt)
    bn = torch.nn.BatchNorm2d(64).to(dev)
    ref = torch.nn.BatchNorm2d(64).double().to(dev)
    with torch.no_grad():
        for m_ in (bn, ref):
            m_.weight.copy_(torch.linspace(0.5, 1.5, 64))
            m_.bias.copy_(torch.linspace(-0.4, 0.2, 64))
            m_.running_mean.copy_(torch.linspace(-0.1, 0.1, 64))
            m_.running_var.copy_(torch.linspace(0.8, 1.2, 64))
    sl = torch.linspace(-0.1, 0.4, npar)
    a = torch.nn.Parameter(sl.to(dev))
    ar = sl.double().to(dev).requires_grad_(True)
    y = A.ops.batch_norm_prelu(x, bn, a)
    assert type(y.grad_fn).__name__ == "BNPReLUFnBackward", "premise: the fused unit"
    y.backward(gy)
    torch.cuda.synchronize()
    # the normalisation is a full-batch reduction: the whole reference runs in float64 on the GPU (torch's own ops), and every
    # image is compared
    xr = _nchw(x.detach().double()).requires_grad_(True)
    yr = F.prelu(ref(xr), ar)
    yr.backward(_nchw(gy.double()))
    _check16(y.detach(), _nhwc(yr.detach()), dt, f"BN + PReLU forward {geom}")
    _check16(x.grad, _nhwc(xr.grad), dt, f"BN + PReLU dx {geom}")
    _check32(bn.weight.grad, ref.weight.grad, f"dgamma {geom}")
    _check32(bn.bias.grad, ref.bias.grad, f"dbeta {geom}")
    _check32(a.grad, ar.grad, f"dslope {geom}")
    _check32(bn.running_mean, ref.running_mean, f"running_mean {geom}")
    _check32(bn.running_var, ref.running_var, f"running_var {geom}")
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 1


@pytest.mark.parametrize("geom", GEOMS)
def test_batchnorm_statistics_well_conditioned_at_bench_batch(A, cus, geom):
    """|mean| >> std (300 +- 0.05, fp32 storage as in test_gpu_batchnorm_prelu.py: the values are not 16-bit numbers) over the
    1024 capped blocks: the one-pass statistics shift by the first pixel, so the variance keeps its digits."""
    n, h, w = _geom(cus, geom)
    _stats_premise(A, n * h * w, geom)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = 300.0 + 0.05 * torch.randn(n, h, w, 64, generator=g, device="cuda")
    bn = torch.nn.BatchNorm2d(64).cuda()
    y = A.ops.batch_norm(x.requires_grad_(True), bn)
    torch.cuda.synchronize()
    xr = x.detach().double().view(-1, 64)
    mean, var = xr.mean(0), xr.var(0, unbiased=False)
    yr = ((xr - mean) / torch.sqrt(var + bn.eps)).view(n, h, w, 64)
    assert float((bn.running_mean.double() - 0.1 * mean).abs().max()) < 1e-4
    assert float((bn.running_var.double() - (0.9 + 0.1 * xr.var(0, unbiased=True))).abs().max() / 0.9) < 1e-5
    err = float((y.detach().double() - yr).abs().max())
    assert err < 2e-2, f"normalised output off by {err}"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. RCAN's channel attention (csrc/ca.hip): srk_ca_pool, srk_ca_apply, srk_ca_bwd_apply, srk_rowsum_group over the batch
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", GEOMS)
def test_rcan_channel_attention(A, cus, dt, geom):
    L = A._lib
    from sr_amd import grads
    n, h, w = _geom(cus, geom)
    HW, C, Cr = h * w, 64, 4
    dev = torch.device("cuda")
    # split_for: ceil(1024 / N) splits of ppb pixels per image, each block walks ppb / 32 rows of 32 pixels
    s = min(max(-(-1024 // n), 1), -(-HW // 64))
    ppb = -(-HW // s)
    ns = int(L.load().srk_ca_splits(n, HW))
    assert ns == -(-HW // ppb) and ns >= 2 and ppb >= 2 * 32, f"premise: {ns} splits of {ppb} pixels"
    if geom == "ragged":
        assert HW % ppb != 0, "premise: the ragged shape has a remainder"
    t = _exd((n, h, w, C), 800 + n, 7, dt)
    x = _exd((n, h, w, C), 810 + n, 7, dt)
    gg = _exd((n, h, w, C), 820 + n, 7, dt)
    w3 = torch.zeros(64, 64, 3, 3, device=dev)
    assert not A.ops.pair_ok(t, w3, w3), "premise: at this batch the model takes the per-layer path with these launches"
    gen = torch.Generator().manual_seed(51)
    cw1, cb1, cw2, cb2 = _ex((Cr, C), gen, 9), _ex((Cr,), gen, 7), _ex((C, Cr), gen, 7), _ex((C,), gen, 7)
    W1, B1, W2, B2 = (v.float().to(dev).contiguous() for v in (cw1, cb1, cw2, cb2))
    st, dtc = A.ops._stream(), A.ops._DT[dt]
    sums, gsum = _nan((n, ns, C), torch.float32), _nan((n, ns, C), torch.float32)
    L.call("srk_ca_pool", L.CaPoolArgs(t=t.data_ptr(), t_pitch=C, t_coff=0, u=0, u_pitch=0, u_coff=0, sums=sums.data_ptr(), N=n, HW=HW, C=C,
                                       dtype=dtc), st)
    L.call("srk_ca_pool", L.CaPoolArgs(t=t.data_ptr(), t_pitch=C, t_coff=0, u=gg.data_ptr(), u_pitch=C, u_coff=0, sums=gsum.data_ptr(),
                                       N=n, HW=HW, C=C, dtype=dtc), st)
    sv, zv, out = _nan((n, C), torch.float32), _nan((n, Cr), torch.float32), _nan((n, h, w, C), dt)
    L.call("srk_ca_apply", L.CaApplyArgs(t=t.data_ptr(), t_pitch=C, t_coff=0, res=x.data_ptr(), res_pitch=C, res_coff=0, sums=sums.data_ptr(),
                                         w1=W1.data_ptr(), b1=B1.data_ptr(), w2=W2.data_ptr(), b2=B2.data_ptr(), s_out=sv.data_ptr(),
                                         z_out=zv.data_ptr(), out=out.data_ptr(), out_pitch=C, out_coff=0, N=n, HW=HW, C=C, Cr=Cr, dtype=dtc,
                                         sums_rows=ns), st)
    K = 2 * Cr * C + Cr + C
    per, gt = _nan((n, K), torch.float32), _nan((n, h, w, C), dt)
    o1, o2, o3 = Cr * C, Cr * C + Cr, 2 * Cr * C + Cr
    L.call("srk_ca_bwd_apply", L.CaBwdArgs(g=gg.data_ptr(), g_pitch=C, g_coff=0, gsum=gsum.data_ptr(), sums=sums.data_ptr(), s=sv.data_ptr(),
                                           z=zv.data_ptr(), w1=W1.data_ptr(), w2=W2.data_ptr(), dw1=per.data_ptr(), db1=per[0, o1:].data_ptr(),
                                           dw2=per[0, o2:].data_ptr(), db2=per[0, o3:].data_ptr(), gt=gt.data_ptr(), gt_pitch=C, gt_coff=0,
                                           N=n, HW=HW, C=C, Cr=Cr, dtype=dtc, sums_rows=ns, gsum_rows=ns), st)
    tot = _nan((K,), torch.float32)
    grads._launch_rowsums([dict(src=per, dst=tot.data_ptr(), n=n, k=K)], st)
    torch.cuda.synchronize()
    # the pooled partials: sums of at most 588 integers k * 2**-7 (or products k k' * 2**-14) are exact in fp32
    tr, gr = t.double().view(n, HW, C), gg.double().view(n, HW, C)
    ref_s = torch.stack([tr[:, j * ppb:(j + 1) * ppb].sum(1) for j in range(ns)], 1)
    ref_g = torch.stack([(tr * gr)[:, j * ppb:(j + 1) * ppb].sum(1) for j in range(ns)], 1)
    assert torch.equal(sums.double(), ref_s), f"ca_pool partials: max err {float((sums.double() - ref_s).abs().max()):.3e}"
    assert torch.equal(gsum.double(), ref_g), f"ca_pool(t * g) partials: max err {float((gsum.double() - ref_g).abs().max()):.3e}"
    # the float64 CALayer (pool -> 1x1 -> ReLU -> 1x1 -> sigmoid) and its backward, per sample
    W1d, B1d, W2d, B2d = (v.to(dev) for v in (cw1, cb1, cw2, cb2))
    m = ref_s.sum(1) / HW
    z = torch.relu(m @ W1d.t() + B1d)
    sg = torch.sigmoid(z @ W2d.t() + B2d)
    _check32(zv, z, f"CA z {geom}")
    _check32(sv, sg, f"CA s {geom}")
    dp2 = ref_g.sum(1) * sg * (1 - sg)
    dp1 = (dp2 @ W2d) * (z > 0)
    dm = dp1 @ W1d / HW
    slots = torch.cat([(dp1[:, :, None] * m[:, None, :]).reshape(n, -1), dp1, (dp2[:, :, None] * z[:, None, :]).reshape(n, -1), dp2], 1)
    _check32(per, slots, f"CA per-sample parameter-gradient slots {geom}")
    # rowsum: the fp32 sum of the GPU's own slots in row order (bound: n roundings of the running sum), and against float64
    pd = per.double()
    bound = n * 2.0 ** -24 * pd.abs().sum(0)
    assert bool(((tot.double() - pd.sum(0)).abs() <= bound + 1e-30).all()), "rowsum of the slots over the batch"
    _check32(tot, slots.sum(0), f"CA parameter gradients {geom}")
    imgs = _pick(n, 1, n, n, seed=n + 7)           # (one image per grid row: first, last, seeded others)
    sgc, dmc = sg[imgs].cpu().view(-1, 1, 1, C), dm[imgs].cpu().view(-1, 1, 1, C)
    _check16(_cpu(out, imgs), _cpu(t, imgs) * sgc + _cpu(x, imgs), dt, f"CA t * s + x {geom} images {imgs}")
    _check16(_cpu(gt, imgs), _cpu(gg, imgs) * sgc + dmc, dt, f"CA data gradient {geom} images {imgs}")


# ------------------------------------------------------------------------------------------------------------------------------
# 5. RDN-B's dense layers (conv_ks_kernel, ncob = 1) on channel slices of the 576-channel concat buffer, their data gradient
#    and grouped weight gradient, and the LFF 1x1 576 -> 64
# ------------------------------------------------------------------------------------------------------------------------------
G0, G, CC = 64, 64, 8
CTOT = G0 + CC * G          # 576


def _ks_premise(cus, n, h, w, geom):
    """conv_ks launch: ncob = CoutP / 64 = 1, min(ntiles, cus) workgroups, workgroup q walks the 16x16 tiles q, q + grid, ..."""
    tiles_img = -(-h // 16) * -(-w // 16)
    nt = n * tiles_img
    ncob = 64 // 64
    grid = min(nt, (cus // ncob) * ncob)
    assert ncob == 1 and nt // grid >= 2, f"premise: {nt} tiles over {grid} workgroups"
    if geom == "ragged":
        assert nt % grid != 0, "premise: the ragged shape has a remainder"
    return tiles_img, nt, grid


def _feat(n, h, w, dt):
    return _exd((n, h, w, CTOT), 1000 + n, 7, dt)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("cin", [128, 320, 512])
def test_rdn_dense_layer_forward_dgrad(A, cus, cache, dt, geom, cin):
    n, h, w = _geom(cus, geom)
    tiles_img, nt, grid = _ks_premise(cus, n, h, w, geom)
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(60 + cin)
    wt, b = _ex((G, cin, 3, 3), gen, 12), _ex((G,), gen, 9)
    wp, bp = torch.nn.Parameter(wt.float().to(dev)), torch.nn.Parameter(b.float().to(dev))
    feat = _feat(n, h, w, dt)
    feat[..., cin:cin + G] = float("nan")
    keep, keep_hi = feat[..., :cin].clone(), feat[..., cin + G:].clone()
    # forward: relu(conv(feat[..., :cin])) written into the next 64-channel slice (what RDBFn.forward launches)
    A.ops.conv_raw(feat[..., :cin], A.ops.pack_conv(wp, bp, dt), N=n, H=h, W=w, Cin=cin, Cout=G, out=feat[..., cin:cin + G], relu=True)
    # data gradient: dy = the slice cin.. of the gradient buffer, accumulated into its prefix with the ReLU mask of slice cin - 64
    gfeat = _exd((n, h, w, CTOT), 1100 + n, 7, dt)
    pref0 = gfeat[..., :cin].clone()
    mask = feat[..., :cin]
    A.ops.conv_raw(gfeat[..., cin:cin + G], A.ops.pack_conv(wp, None, dt, dgrad=True), N=n, H=h, W=w, Cin=G, Cout=cin, out=gfeat[..., :cin],
                   res=gfeat[..., :cin], mask=mask, mask_from=cin - G, use_bias=False)
    torch.cuda.synchronize()
    assert torch.equal(feat[..., :cin], keep) and torch.equal(feat[..., cin + G:], keep_hi), "the forward wrote outside its slice"
    assert bool(torch.isfinite(feat[..., cin:cin + G]).all()), "an output tile was never written"
    imgs = _pick_strided(n, tiles_img, nt, grid, seed=n + cin)
    key = ("ks", geom, cin)
    if key not in cache:
        xs = _nchw(_cpu(feat[..., :cin], imgs))
        fwd = _nhwc(torch.relu(F.conv2d(xs, wt, b, padding=1)))
        dy = _nchw(_cpu(gfeat[..., cin:cin + G], imgs))
        cache[key] = (fwd, _nhwc(F.conv_transpose2d(dy, wt, padding=1)))
    fwd, dg = cache[key]
    got = _cpu(feat[..., cin:cin + G], imgs)
    assert bool((got[fwd == 0] == 0).all()), "ReLU-zeroed elements are exactly zero"
    _check16(got, fwd, dt, f"dense conv {cin}->64 {geom} images {imgs}")
    ref = dg + _cpu(pref0, imgs)
    m_ = _cpu(mask, imgs) > 0
    m_[..., :cin - G] = True
    ref = torch.where(m_, ref, torch.zeros((), dtype=torch.float64))
    _check16(_cpu(gfeat[..., :cin], imgs), ref, dt, f"dense conv {cin}->64 dgrad {geom} images {imgs}")


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", GEOMS)
def test_rdn_dense_layer_wgrad_and_lff(A, cus, cache, dt, geom):
    n, h, w = _geom(cus, geom)
    cin = 320
    tiles_img, nt, grid = _ks_premise(cus, n, h, w, geom)
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(70)
    wt, b = _ex((G, cin, 3, 3), gen, 12), _ex((G,), gen, 9)
    wl, bl = _ex((G0, CTOT, 1, 1), gen, 12), _ex((G0,), gen, 9)
    wp, bp = torch.nn.Parameter(wt.float().to(dev)), torch.nn.Parameter(b.float().to(dev))
    feat = _feat(n, h, w, dt)
    dy = _exd((n, h, w, CTOT), 1200 + n, 7, dt)[..., cin:cin + G]        # a channel slice of the gradient buffer, as in RDBFn
    with A.ops.hold_wgrads():
        gw, gb = A.ops.wgrad(feat[..., :cin], dy, wparam=wp, bparam=bp, N=n, H=h, W=w, Cin=cin, Cout=G, k=3, w_shape=(G, cin, 3, 3),
                             want_bias=True)
        assert len(A.ops._WQ.jobs) == 1, "premise: the weight gradient is a grouped-ring job"
    # LFF: 1x1 over the whole buffer + the block input (conv1x1.hip)
    x = _exd((n, h, w, G0), 1300 + n, 7, dt)
    out = _nan((n, h, w, G0), dt)
    A.ops.conv_raw(feat, A.ops.pack_conv(torch.nn.Parameter(wl.float().to(dev)), torch.nn.Parameter(bl.float().to(dev)), dt),
                   N=n, H=h, W=w, Cin=CTOT, Cout=G0, out=out, res=x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "an LFF output tile was never written"
    key = ("ksw", geom)
    if key not in cache:
        rw = torch.zeros(G, cin, 3, 3, dtype=torch.float64, device=dev)
        for n0 in range(0, n, CHUNK):
            rw += torch.nn.grad.conv2d_weight(_nchw(feat[n0:n0 + CHUNK, ..., :cin].double()), (G, cin, 3, 3), _nchw(dy[n0:n0 + CHUNK].double()),
                                              padding=1)
        cache[key] = (rw.cpu(), dy.double().sum((0, 1, 2)).cpu())
    rw, rb = cache[key]
    _check32(gw, rw, f"dense conv 320->64 dW {geom}")
    _check32(gb, rb, f"dense conv 320->64 db {geom}")
    imgs = _pick(n, tiles_img, nt, grid, seed=n + 9)
    ref = _cpu(feat, imgs).reshape(-1, CTOT) @ wl.view(G0, CTOT).t() + bl + _cpu(x, imgs).reshape(-1, G0)
    _check16(_cpu(out, imgs).reshape(-1, G0), ref, dt, f"LFF 576->64 {geom} images {imgs}")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. WDSR-B's pointwise pair 128 -> 768 -> 102 (csrc/pw_chain.hip): forward, backward, weight gradient over pixel ranges + finalize
# ------------------------------------------------------------------------------------------------------------------------------
PF, PH, PM = 128, 768, 102


def _pw_operands(A, n, h, w, dt):
    gen = torch.Generator().manual_seed(80)
    w1, b1 = _ex((PH, PF, 1, 1), gen, 12), _ex((PH,), gen, 9)
    w2, b2 = _ex((PM, PH, 1, 1), gen, 12), _ex((PM,), gen, 9)
    P = n * h * w
    x = _exd((1, 1, P, PF), 1400 + n, 7, dt)
    cz = A.ops.pad16(PM)
    gz = _exd((1, 1, P, cz), 1500 + n, 7, dt)
    gz[..., PM:] = 0
    res = _exd((1, 1, P, PF), 1600 + n, 7, dt)
    return w1, b1, w2, b2, x, gz, res


def _pw_ref(x, gz, w1, b1, w2, b2, dt):
    """The float64 statement of test_gpu_pw_chain.py (h and gh rounded to the storage type where the kernels store / feed them)."""
    pre = x @ w1.view(PH, PF).t() + b1
    hr = torch.relu(pre).to(dt).double()
    zr = hr @ w2.view(PM, PH).t() + b2
    ghr = ((gz @ w2.view(PM, PH)) * (pre > 0)).to(dt).double()
    return hr, zr, ghr


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("geom", GEOMS)
def test_wdsr_pointwise_pair(A, cus, cache, dt, geom):
    L = A._lib
    n, h, w = _geom(cus, geom)
    P, HWi = n * h * w, h * w
    dev = torch.device("cuda")
    w1, b1, w2, b2, x, gz, res = _pw_operands(A, n, h, w, dt)
    # srk_pw_wgrad: NR ranges of 64-pixel tiles, range r walks tq (+1) of them
    ntiles = -(-P // 64)
    nr = int(L.load().srk_pw_wgrad_ranges(P, PH))
    tq, trem = divmod(ntiles, nr)
    assert tq >= 2 and nr >= 8, f"premise: {ntiles} tiles over {nr} ranges"
    if geom == "ragged":
        assert trem != 0 and P % 64 != 0, "premise: the ragged shape has a remainder (and a partial last tile)"
    pk = A.ops.pw_pack(torch.nn.Parameter(w1.float().to(dev)), b1.float().to(dev), torch.nn.Parameter(w2.float().to(dev)),
                       b2.float().to(dev), dt)
    cz = gz.shape[3]
    z = _nan((1, 1, P, cz), dt)
    A.ops.pw_forward_raw(x, pk, z)
    gx, hid, ghid = _nan((1, 1, P, PF), dt), _nan((1, 1, P, PH), dt), _nan((1, 1, P, PH), dt)
    A.ops.pw_backward_raw(x, gz, pk, gx, res=res, h_out=hid, gh_out=ghid)
    # the weight gradient as pw_wgrad_raw launches it, with NaN-filled range partials and outputs
    scratch = _nan((nr * (pk.chid * (pk.cin + pk.coutp + 1) + pk.coutp),), torch.float32)
    dw1, dw2 = _nan((PH, PF, 1, 1), torch.float32), _nan((PM, PH, 1, 1), torch.float32)
    db1, db2 = _nan((PH,), torch.float32), _nan((PM,), torch.float32)
    o2 = nr * pk.chid * pk.cin
    o3 = o2 + nr * pk.chid * pk.coutp
    o4 = o3 + nr * pk.chid
    sp = scratch.data_ptr()
    L.call("srk_pw_wgrad", L.PwWgradArgs(
        x=x.data_ptr(), x_pitch=PF, x_coff=0, gz=gz.data_ptr(), gz_pitch=cz, gz_coff=0, Cz=cz, P=P, Cin=pk.cin, Chid=pk.chid, Cmid=pk.cmid,
        CoutP=pk.coutp, wpk=pk.bwd.data_ptr(), dw1p=sp, dw2p=sp + 4 * o2, db1p=sp + 4 * o3, db2p=sp + 4 * o4, nranges=nr,
        dw1=dw1.data_ptr(), db1=db1.data_ptr(), dw2=dw2.data_ptr(), db2=db2.data_ptr(), dtype=A.ops._DT[dt]), A.ops._stream())
    torch.cuda.synchronize()
    for t_, name in ((z, "z"), (gx, "gx"), (hid, "h"), (ghid, "gh")):
        assert bool(torch.isfinite(t_).all()), f"{name}: a tile was never written"
    assert float(z[..., PM:].abs().max()) == 0.0, "padding channels are zeros"
    # per image (2304 pixels) on the CPU: the images holding the first tile of the ranges trem - 1 and trem, ...
    first = lambda r: (r * tq + min(r, trem)) * 64 // HWi             # noqa: E731  the image holding range r's first tile
    imgs = sorted(set(_pick(n, 1, n, n, seed=n + 11)[:13]) | {first(trem - 1), first(trem), first(nr - 1)})
    rows = torch.cat([torch.arange(i * HWi, (i + 1) * HWi) for i in imgs])
    xs, gzs = x.view(P, PF)[rows].double().cpu(), gz.view(P, cz)[rows, :PM].double().cpu()
    hr, zr, ghr = _pw_ref(xs, gzs, w1, b1, w2, b2, dt)
    what = f"{geom} images {imgs}"
    _check16(hid.view(P, PH)[rows].cpu(), hr, dt, f"pw h {what}")
    _check16(z.view(P, cz)[rows, :PM].cpu(), zr, dt, f"pw z {what}")
    _check16(ghid.view(P, PH)[rows].cpu(), ghr, dt, f"pw gh {what}")
    _check16(gx.view(P, PF)[rows].cpu(), ghr @ w1.view(PH, PF) + res.view(P, PF)[rows].double().cpu(), dt, f"pw gx {what}")
    key = ("pw", geom, dt)                          # (the reference rounds h and gh to the storage type)
    if key not in cache:
        W1, B1, W2, B2 = (v.to(dev) for v in (w1, b1, w2, b2))
        r1 = torch.zeros(PH, PF, dtype=torch.float64, device=dev)
        r2 = torch.zeros(PM, PH, dtype=torch.float64, device=dev)
        rb1 = torch.zeros(PH, dtype=torch.float64, device=dev)
        step = CHUNK * HWi
        for p0 in range(0, P, step):
            xc, gc = x.view(P, PF)[p0:p0 + step].double(), gz.view(P, cz)[p0:p0 + step, :PM].double()
            hc, _, ghc = _pw_ref(xc, gc, W1, B1, W2, B2, dt)
            r1 += ghc.t() @ xc
            r2 += gc.t() @ hc
            rb1 += ghc.sum(0)
        cache[key] = (r1.cpu(), rb1.cpu(), r2.cpu(), gz.view(P, cz)[:, :PM].double().sum(0).cpu())
    r1, rb1, r2, rb2 = cache[key]
    _check32(dw1.view(PH, PF), r1, f"pw dW1 {geom}")
    _check32(db1, rb1, f"pw db1 {geom}")
    _check32(dw2.view(PM, PH), r2, f"pw dW2 {geom}")
    _check32(db2, rb2, f"pw db2 {geom}")
