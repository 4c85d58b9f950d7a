"""D-DBPN's column path -- the main path of its 33 projection convolutions at scales 2 and 8 and in every fp32 run -- piece by piece
against float64: srk_unfold_nhwc / srk_fold_nhwc (csrc/generic.hip) bit for bit, then ops.conv_general / ops.conv_transpose_general
(ops_proj.py: UnfoldFn / FoldFn around a 1x1 GEMM 1152 - 4608 channels wide) stage by stage.  Geometries (kernel, stride, padding):
(6,2,2), (8,4,2), (12,8,2) of models/ddbpn.py `projection_conv`; operands are the exact ones of geometry_ref._ex (integers
|k| <= 127 times 2**-7, weights times 2**-12), so the im2col is a copy, the col2im sums at most ceil(K/s)**2 (9 or 4) column values and
an fp32 bias exactly in fp32 and rounds ONCE, and both must EQUAL the reference.  Outputs are prefilled with NaN.

Why stage by stage: a transposed conv here stores the GEMM's column tensor in 16 bits and then adds up to 9 of its entries (a strided
conv's data gradient likewise), so it differs from ONE float64 conv_transpose2d by several half-ulps of the partial sums.  The reference
follows the code's stages: the column tensor handed to the fold is recorded (a wrapper around ops_proj._fold_raw), the GEMM is checked
per element (geometry_ref._check16) against a float64 einsum over the OIHW / IOHW weight, the fold exactly from the recorded columns.
The one-rounding results (strided forward, transposed data gradient) are checked against float64 conv2d directly."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geometry_ref import _check16, _check32, _ex  # noqa: E402

pytestmark = pytest.mark.gpu

GEOMS = [(6, 2, 2), (8, 4, 2), (12, 8, 2)]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
C, N = 32, 2
GRID_CAP = 2048 * 256           # both launchers: at most 2048 blocks of 256 threads, each thread strides over the work items


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _chunk(dt):
    return 4 if dt == torch.float32 else 8          # elements of a 16-byte access


def _nan(shape, dt):
    return torch.full(tuple(shape), float("nan"), dtype=dt, device="cuda")


def _unfold_extents(k, s, p):
    """(H, W) of the inputs: windows that all reach into the padding, tile multiples, and a size that is no multiple: the floor in Ho / Wo, and from stride 4 on last columns that no window covers."""
    return [(s * lh, s * lw) for lh, lw in ((1, 1), (3, 2), (5, 7))] + [(s * 3 + 1, s * 2 + s - 1)]


def _out_hw(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _call_unfold(A, x, cols, *, h, w, k, s, p, c=C, x_pitch=None, x_coff=0, cols_pitch=None, n=N):
    L = A._lib
    ho, wo = _out_hw(h, w, k, s, p)
    L.call("srk_unfold_nhwc", L.UnfoldNhwcArgs(x=x.data_ptr(), x_pitch=c if x_pitch is None else x_pitch, x_coff=x_coff, cols=cols.data_ptr(),
                                               cols_pitch=k * k * c if cols_pitch is None else cols_pitch, N=n, H=h, W=w, C=c, K=k, stride=s,
                                               pad=p, Ho=ho, Wo=wo, dtype=A.ops._DT[x.dtype]), A.ops._stream())
    torch.cuda.synchronize()


def _call_fold(A, cols, bias, out, *, hi, wi, ho, wo, k, s, p, c=C, cols_pitch=None, out_pitch=None, out_coff=0, n=N):
    L = A._lib
    L.call("srk_fold_nhwc", L.FoldNhwcArgs(cols=cols.data_ptr(), cols_pitch=k * k * c if cols_pitch is None else cols_pitch,
                                           bias=0 if bias is None else bias.data_ptr(), out=out.data_ptr(), out_pitch=c if out_pitch is None else out_pitch,
                                           out_coff=out_coff, N=n, Hi=hi, Wi=wi, C=c, K=k, stride=s, pad=p, Ho=ho, Wo=wo,
                                           dtype=A.ops._DT[cols.dtype]), A.ops._stream())
    torch.cuda.synchronize()


def _unfold_ref(x, k, s, p):
    """NHWC float tensor -> F.unfold reordered to the kernel's [(kh*K + kw)*C + c] layout (same dtype as `x`: a copy either way)."""
    n, h, w, c = x.shape
    ho, wo = _out_hw(h, w, k, s, p)
    u = F.unfold(x.permute(0, 3, 1, 2), k, stride=s, padding=p)                  # [n, c*k*k, ho*wo], channel index (c, kh, kw)
    return u.reshape(n, c, k * k, ho, wo).permute(0, 3, 4, 2, 1).reshape(n, ho, wo, k * k * c)


def _fold_ref(cols, bias, ho, wo, k, s, p):
    """The sum of the column entries per output element (+ bias), in the arithmetic of `cols` (float64; float32 where that is exact)."""
    n, hi, wi, kkc = cols.shape
    c = kkc // (k * k)
    u = cols.reshape(n, hi * wi, k * k, c).permute(0, 3, 2, 1).reshape(n, c * k * k, hi * wi)
    out = F.fold(u, (ho, wo), k, stride=s, padding=p).permute(0, 2, 3, 1)
    return out if bias is None else out + bias.to(out.dtype)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. the two kernels, bit for bit
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "k%ds%dp%d" % g)
def test_unfold_is_a_copy(A, geom, dt):
    k, s, p = geom
    g = torch.Generator().manual_seed(100 * k + s)
    for h, w in _unfold_extents(k, s, p):
        x = _ex((N, h, w, C), g, 7)
        ho, wo = _out_hw(h, w, k, s, p)
        cols = _nan((N, ho, wo, k * k * C), dt)
        _call_unfold(A, x.to(dt).cuda(), cols, h=h, w=w, k=k, s=s, p=p)
        ref = _unfold_ref(x, k, s, p)
        assert torch.equal(cols.double().cpu(), ref), f"{h}x{w}: {int((cols.double().cpu() != ref).sum())} of {ref.numel()} elements differ"


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "k%ds%dp%d" % g)
def test_fold_is_the_float64_sum_rounded_once(A, geom, dt, bias):
    k, s, p = geom
    g = torch.Generator().manual_seed(200 * k + s + int(bias))
    # (Hi, Wi, Ho, Wo): the transposed conv's extents, and what UnfoldFn.backward asks for -- the gradient of an input the windows do not
    # cover completely: from stride 4 on its last s - 3 columns receive nothing and must come out as exact zeros (the bias alone)
    cases = [(hi, wi, (hi - 1) * s - 2 * p + k, (wi - 1) * s - 2 * p + k) for hi, wi in ((1, 1), (3, 2), (5, 7))]
    cases += [(*_out_hw(h, w, k, s, p), h, w) for h, w in _unfold_extents(k, s, p)]
    for hi, wi, ho, wo in cases:
        cols = _ex((N, hi, wi, k * k * C), g, 7)
        b = _ex((C,), g, 7) if bias else None
        out = _nan((N, ho, wo, C), dt)
        _call_fold(A, cols.to(dt).cuda(), None if b is None else b.float().cuda(), out, hi=hi, wi=wi, ho=ho, wo=wo, k=k, s=s, p=p)
        ref = _fold_ref(cols, b, ho, wo, k, s, p)
        assert torch.equal(ref.float().double(), ref)                # <= 9 terms of 8 bits + the bias: exact in fp32, the kernel rounds once
        ref = ref.to(dt)
        assert torch.equal(out.cpu(), ref), f"{hi}x{wi} -> {ho}x{wo}: {int((out.cpu() != ref).sum())} of {ref.numel()} elements differ"
        last = (wi - 1) * s - p + k                                   # first column right of the last window
        if (ho, wo) == (s * 3 + 1, s * 2 + s - 1) and s > 2:          # (every row is covered, and at stride 2 every column)
            edge = out[:, :, last:].float().cpu()
            assert edge.shape[2] == s - 3 and torch.equal(edge, (torch.zeros(C) if b is None else b.float()).expand_as(edge).to(dt).float())


def test_unfold_grid_stride_walk(A):
    """More work items than the capped grid has threads: every thread takes a second item, the last pass is ragged."""
    k, s, p = 6, 2, 2
    dt = torch.bfloat16
    h, w = 96, 82
    ho, wo = _out_hw(h, w, k, s, p)
    total = N * ho * wo * k * k * (C // _chunk(dt))
    assert GRID_CAP < total < 2 * GRID_CAP and total % GRID_CAP
    x = _ex((N, h, w, C), torch.Generator().manual_seed(5), 7)
    cols = _nan((N, ho, wo, k * k * C), dt)
    _call_unfold(A, x.to(dt).cuda(), cols, h=h, w=w, k=k, s=s, p=p)
    assert torch.equal(cols.float().cpu(), _unfold_ref(x.float(), k, s, p))


def test_fold_grid_stride_walk(A):
    k, s, p = 6, 2, 2
    dt = torch.bfloat16
    hi, wi = 130, 127
    ho, wo = (hi - 1) * s - 2 * p + k, (wi - 1) * s - 2 * p + k
    total = N * ho * wo * (C // _chunk(dt))
    assert GRID_CAP < total < 2 * GRID_CAP and total % GRID_CAP
    g = torch.Generator().manual_seed(6)
    cols = torch.randint(-127, 128, (N, hi, wi, k * k * C), generator=g, dtype=torch.int16).to(dt) * 2.0 ** -7       # geometry_ref._ex's values
    b = _ex((C,), g, 7).float()
    out = _nan((N, ho, wo, C), dt)
    _call_fold(A, cols.cuda(), b.cuda(), out, hi=hi, wi=wi, ho=ho, wo=wo, k=k, s=s, p=p)
    ref = _fold_ref(cols.float(), b, ho, wo, k, s, p)               # 9 terms of 8 bits + the bias: float32 is exact, as float64 is
    assert torch.equal(out.cpu(), ref.to(dt))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS.get)
def test_unfold_pitch_and_offset_fields(A, dt):
    """x_pitch / x_coff / cols_pitch, which ops_proj never sets: a 32-channel slice at offset 16 of a 64-channel tensor, a column tensor
    with 16 spare channels per pixel that must keep their prefill."""
    k, s, p = 6, 2, 2
    h, w = 6, 10
    g = torch.Generator().manual_seed(7)
    x = _ex((N, h, w, 64), g, 7)
    ho, wo = _out_hw(h, w, k, s, p)
    pitch = k * k * C + 16
    cols = _nan((N, ho, wo, pitch), dt)
    _call_unfold(A, x.to(dt).cuda(), cols, h=h, w=w, k=k, s=s, p=p, x_pitch=64, x_coff=16, cols_pitch=pitch)
    assert torch.equal(cols[..., :k * k * C].double().cpu(), _unfold_ref(x[..., 16:48].contiguous(), k, s, p))
    assert bool(torch.isnan(cols[..., k * k * C:]).all()), "the spare channels of the column tensor were written"


@pytest.mark.parametrize("dt", DTYPES, ids=IDS.get)
def test_fold_pitch_and_offset_fields(A, dt):
    """cols_pitch / out_pitch / out_coff: spare column channels that must not be read, an output slice at offset 16 of a 64-channel tensor
    whose other channels keep their prefill."""
    k, s, p = 6, 2, 2
    hi, wi = 3, 5
    ho, wo = (hi - 1) * s - 2 * p + k, (wi - 1) * s - 2 * p + k
    g = torch.Generator().manual_seed(8)
    pitch = k * k * C + 16
    cols = _ex((N, hi, wi, pitch), g, 7)
    b = _ex((C,), g, 7)
    out = _nan((N, ho, wo, 64), dt)
    _call_fold(A, cols.to(dt).cuda(), b.float().cuda(), out, hi=hi, wi=wi, ho=ho, wo=wo, k=k, s=s, p=p, cols_pitch=pitch, out_pitch=64, out_coff=16)
    ref = _fold_ref(cols[..., :k * k * C].contiguous(), b, ho, wo, k, s, p).to(dt)
    assert torch.equal(out[..., 16:48].cpu(), ref)
    assert bool(torch.isnan(out[..., :16]).all()) and bool(torch.isnan(out[..., 48:]).all()), "channels outside the addressed slice were written"


# --------------------------------------------------------------------------------------------------------------------------------
# 2. conv_general / conv_transpose_general on the column path, stage by stage
# --------------------------------------------------------------------------------------------------------------------------------
def _record_folds(A, monkeypatch):
    """Wraps ops_proj._fold_raw: [(column tensor, bias, output)] of every fold the ops launch."""
    rec = []
    real = A.ops_proj._fold_raw

    def spy(cols, c, k, stride, pad, ho, wo, bias=None):
        out = real(cols, c, k, stride, pad, ho, wo, bias)
        rec.append((cols.detach().clone(), None if bias is None else bias.detach().clone(), out.detach().clone()))
        return out
    monkeypatch.setattr(A.ops_proj, "_fold_raw", spy)
    return rec


def _check_fold_stage(rec, dt, ho, wo, k, s, p, what):
    """The recorded fold against the float64 sum of ITS OWN columns: exact in 16 bits (test_fold_is_the_float64_sum_rounded_once)."""
    cols, bias, out = rec
    cols, bias = cols.double().cpu(), None if bias is None else bias.double().cpu()
    ref = _fold_ref(cols, bias, ho, wo, k, s, p)
    if dt == torch.float32:
        _check32(out, ref, what + " (fold)")
    else:
        # premise of "exact": the columns are 16-bit roundings of multiples of 2**-19 (8-bit operands times 2**-7 and 2**-12), the bias
        # is one of 2**-7, and the absolute values of a sum's terms stay below 2**5: every partial sum fits fp32's 24 bits
        assert torch.equal((cols * 2.0 ** 19).round(), cols * 2.0 ** 19)
        assert float(_fold_ref(cols.abs(), None if bias is None else bias.abs(), ho, wo, k, s, p).max()) < 32
        assert torch.equal(out.cpu(), ref.to(dt)), f"{what} (fold): {int((out.cpu() != ref.to(dt)).sum())} of {ref.numel()} elements differ"


def _check(got, ref, dt, what):
    if dt == torch.float32:
        _check32(got, ref, what)
    else:
        _check16(got.cpu(), ref, dt, what)


def _column_path(A, monkeypatch, x, w, stride, pad, up):
    """At scale 4 in 16 bits the direct kernels would answer: switch them off, and make sure of it."""
    if stride == 4 and x.dtype != torch.float32:
        monkeypatch.setattr(A.ops_proj, "_PROJ_OFF", True)
    assert not A.ops.proj_ok(x, w, stride, pad, up)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("lr", [(5, 7), (1, 1)], ids=["5x7", "1x1"])          # 2 * 5 * 7 = 70 LR pixels: one full 64-pixel GEMM tile and a remainder
@pytest.mark.parametrize("dt", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "k%ds%dp%d" % g)
def test_strided_conv_stage_by_stage(A, monkeypatch, geom, dt, lr, bias):
    k, s, p = geom
    lh, lw = lr
    h, wd = s * lh, s * lw
    g = torch.Generator().manual_seed(1000 * k + 10 * lh + int(bias))
    x, w, gy = _ex((N, h, wd, C), g, 7), _ex((C, C, k, k), g, 12), _ex((N, lh, lw, C), g, 7)
    b = _ex((C,), g, 7) if bias else None
    xd = x.to(dt).cuda().requires_grad_(True)
    wp = w.float().cuda().requires_grad_(True)
    bp = b.float().cuda().requires_grad_(True) if bias else None
    _column_path(A, monkeypatch, xd, wp, s, p, False)
    rec = _record_folds(A, monkeypatch)
    y = A.ops.conv_general(xd, wp, bp, stride=s, pad=p)
    assert A._lib.load().srk_last_kernel().decode() == "conv_igemm<32,1>"       # the streaming 1x1 kernel over K*K*32 input channels
    assert tuple(y.shape) == (N, lh, lw, C) and not rec
    xn, gn = x.permute(0, 3, 1, 2), gy.permute(0, 3, 1, 2)
    _check(y.detach().permute(0, 3, 1, 2), F.conv2d(xn, w, b, stride=s, padding=p), dt, "strided conv forward")           # one rounding
    y.backward(gy.to(dt).cuda())
    A.ops.flush_wgrads()
    torch.cuda.synchronize()
    # data gradient: GEMM to K*K*32 columns (stored), then the fold
    assert len(rec) == 1 and tuple(rec[0][0].shape) == (N, lh, lw, k * k * C) and rec[0][1] is None
    _check(rec[0][0], torch.einsum("nhwo,oikl->nhwkli", gy, w).reshape(N, lh, lw, k * k * C), dt, "strided conv data gradient (GEMM)")
    _check_fold_stage(rec[0], dt, h, wd, k, s, p, "strided conv data gradient")
    assert torch.equal(xd.grad, rec[0][2]) and tuple(xd.grad.shape) == (N, h, wd, C)
    assert tuple(wp.grad.shape) == (C, C, k, k)
    _check32(wp.grad, torch.nn.grad.conv2d_weight(xn, (C, C, k, k), gn, stride=s, padding=p), "strided conv weight gradient")
    if bias:
        _check32(bp.grad, gn.sum(dim=(0, 2, 3)), "strided conv bias gradient")


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("lr", [(5, 7), (1, 1)], ids=["5x7", "1x1"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "k%ds%dp%d" % g)
def test_transposed_conv_stage_by_stage(A, monkeypatch, geom, dt, lr, bias):
    k, s, p = geom
    lh, lw = lr
    h, wd = (lh - 1) * s - 2 * p + k, (lw - 1) * s - 2 * p + k
    g = torch.Generator().manual_seed(2000 * k + 10 * lh + int(bias))
    x, w, gy = _ex((N, lh, lw, C), g, 7), _ex((C, C, k, k), g, 12), _ex((N, h, wd, C), g, 7)          # w: [in][out][K][K]
    b = _ex((C,), g, 7) if bias else None
    xd = x.to(dt).cuda().requires_grad_(True)
    wp = w.float().cuda().requires_grad_(True)
    bp = b.float().cuda().requires_grad_(True) if bias else None
    _column_path(A, monkeypatch, xd, wp, s, p, True)
    rec = _record_folds(A, monkeypatch)
    y = A.ops.conv_transpose_general(xd, wp, bp, stride=s, pad=p)
    assert A._lib.load().srk_last_kernel().decode() == "conv_igemm<128,1>"      # ... to K*K*32 = 1152 / 2048 / 4608 output channels
    assert tuple(y.shape) == (N, h, wd, C) == (N, s * lh, s * lw, C)
    # forward: GEMM to the column tensor (stored), then the fold with the bias
    assert len(rec) == 1 and tuple(rec[0][0].shape) == (N, lh, lw, k * k * C) and (rec[0][1] is not None) == bias
    _check(rec[0][0], torch.einsum("nhwi,iokl->nhwklo", x, w).reshape(N, lh, lw, k * k * C), dt, "transposed conv forward (GEMM)")
    if bias:
        assert torch.equal(rec[0][1].double().cpu(), b)
    _check_fold_stage(rec[0], dt, h, wd, k, s, p, "transposed conv forward")
    assert torch.equal(y.detach(), rec[0][2])
    y.backward(gy.to(dt).cuda())
    A.ops.flush_wgrads()
    torch.cuda.synchronize()
    assert len(rec) == 1
    xn, gn = x.permute(0, 3, 1, 2), gy.permute(0, 3, 1, 2)
    assert tuple(xd.grad.shape) == (N, lh, lw, C)
    _check(xd.grad.permute(0, 3, 1, 2), F.conv2d(gn, w, None, stride=s, padding=p), dt, "transposed conv data gradient")   # unfold + GEMM: one rounding
    assert tuple(wp.grad.shape) == (C, C, k, k)
    # the transposed conv is the adjoint of conv2d(., w): its weight gradient is that conv's, with input and output gradient swapped
    _check32(wp.grad, torch.nn.grad.conv2d_weight(gn, (C, C, k, k), xn, stride=s, padding=p), "transposed conv weight gradient")
    if bias:
        _check32(bp.grad, gn.sum(dim=(0, 2, 3)), "transposed conv bias gradient")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS.get)
def test_strided_conv_with_padded_input_channels(A, monkeypatch, dt):
    """conv_general's `cp != cin` branch: a 20-input-channel weight on a 32-channel tensor whose channels 20.. are the zero padding."""
    k, s, p = 6, 2, 2
    lh, lw, cin = 5, 7, 20
    h, wd = s * lh, s * lw
    g = torch.Generator().manual_seed(31)
    x = _ex((N, h, wd, C), g, 7)
    x[..., cin:] = 0
    w, b, gy = _ex((C, cin, k, k), g, 12), _ex((C,), g, 7), _ex((N, lh, lw, C), g, 7)
    xd = x.to(dt).cuda().requires_grad_(True)
    wp, bp = w.float().cuda().requires_grad_(True), b.float().cuda().requires_grad_(True)
    rec = _record_folds(A, monkeypatch)
    y = A.ops.conv_general(xd, wp, bp, stride=s, pad=p)
    xn, gn = x.permute(0, 3, 1, 2)[:, :cin], gy.permute(0, 3, 1, 2)
    _check(y.detach().permute(0, 3, 1, 2), F.conv2d(xn, w, b, stride=s, padding=p), dt, "forward")
    y.backward(gy.to(dt).cuda())
    A.ops.flush_wgrads()
    torch.cuda.synchronize()
    gcols = torch.einsum("nhwo,oikl->nhwkli", gy, F.pad(w, (0, 0, 0, 0, 0, C - cin))).reshape(N, lh, lw, k * k * C)
    _check(rec[0][0], gcols, dt, "data gradient (GEMM)")
    _check_fold_stage(rec[0], dt, h, wd, k, s, p, "data gradient")
    assert torch.equal(xd.grad[..., cin:], torch.zeros_like(xd.grad[..., cin:])), "the padding channels' gradient is not exactly 0"
    assert tuple(wp.grad.shape) == (C, cin, k, k) and tuple(bp.grad.shape) == (C,)
    _check32(wp.grad, torch.nn.grad.conv2d_weight(xn, (C, cin, k, k), gn, stride=s, padding=p), "weight gradient")
    _check32(bp.grad, gn.sum(dim=(0, 2, 3)), "bias gradient")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS.get)
def test_transposed_conv_with_padded_output_channels(A, monkeypatch, dt):
    """conv_transpose_general's `coutp != cout` branch: 3 output channels stored as 16, channels 3.. exactly 0."""
    k, s, p = 6, 2, 2
    lh, lw, cout, coutp = 5, 7, 3, 16
    h, wd = s * lh, s * lw
    g = torch.Generator().manual_seed(32)
    x, w, b = _ex((N, lh, lw, C), g, 7), _ex((C, cout, k, k), g, 12), _ex((cout,), g, 7)
    gy = _ex((N, h, wd, coutp), g, 7)
    gy[..., cout:] = 0
    xd = x.to(dt).cuda().requires_grad_(True)
    wp, bp = w.float().cuda().requires_grad_(True), b.float().cuda().requires_grad_(True)
    rec = _record_folds(A, monkeypatch)
    y = A.ops.conv_transpose_general(xd, wp, bp, stride=s, pad=p)
    assert tuple(y.shape) == (N, h, wd, coutp)
    assert torch.equal(y.detach()[..., cout:], torch.zeros_like(y.detach()[..., cout:])), "the padding channels are not exactly 0"
    cols = torch.einsum("nhwi,iokl->nhwklo", x, F.pad(w, (0, 0, 0, 0, 0, coutp - cout))).reshape(N, lh, lw, k * k * coutp)
    _check(rec[0][0], cols, dt, "forward (GEMM)")
    assert torch.equal(rec[0][1].double().cpu(), F.pad(b, (0, coutp - cout)))
    _check_fold_stage(rec[0], dt, h, wd, k, s, p, "forward")
    assert torch.equal(y.detach(), rec[0][2])
    y.backward(gy.to(dt).cuda())
    A.ops.flush_wgrads()
    torch.cuda.synchronize()
    xn, gn = x.permute(0, 3, 1, 2), gy.permute(0, 3, 1, 2)[:, :cout]
    _check(xd.grad.permute(0, 3, 1, 2), F.conv2d(gn, w, None, stride=s, padding=p), dt, "data gradient")
    assert tuple(wp.grad.shape) == (C, cout, k, k) and tuple(bp.grad.shape) == (cout,)
    _check32(wp.grad, torch.nn.grad.conv2d_weight(gn, (C, cout, k, k), xn, stride=s, padding=p), "weight gradient")
    _check32(bp.grad, gn.sum(dim=(0, 2, 3)), "bias gradient")
