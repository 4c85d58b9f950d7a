"""Tiled and x8 self-ensemble inference on the GPU (sr_amd.tiling, csrc/tile.hip, SRModel(tile=..., self_ensemble=...)).

* srk_tile_gather / srk_tile_place alone against torch indexing, bit for bit (they only move fp32 values; the accumulate mode adds
  0.125 * v, and multiplying by 0.125 is exact);
* every model with a HIP path through predict_step / validation_step with tile=24, tile_pad=8, tile_batch=5 on LR 45 x 59, against the
  independent float64 statement (tests/tiling_ref.py) wrapped around the float64 oracle, judged by eval_ref.check_image with its own limits
  and floors (its row / column statistics are what catch a misplaced seam);
* self-ensemble on and off, alone and with tiling: same judge; two runs are bit-identical;
* both options off: the parent path's image, bit for bit.
Every case prints `EVAL ...` lines: measured value next to limit (run with -s to keep them)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_ref as ER  # noqa: E402
import tiling_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

TILE, PAD, BATCH = 24, 8, 5
H, W = 45, 59


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------------------------------------------------------------
def _entries(A, h, w, scale, pad):
    """Every (k, tile) of the 8 transformed grids of an h x w image: (k, plan, tile), in the order k = 0..7."""
    out = []
    for k in range(8):
        p = A.tiling.plan(w, h, scale, TILE, pad) if k & 4 else A.tiling.plan(h, w, scale, TILE, pad)
        out += [(k, p, t) for t in p.tiles]
    return out


def _owned_in_image(k, p, t):
    """The owned HR rectangle of tile t (rows / columns of the TRANSFORMED HR frame) as (y, x, h, w) of the untransformed HR image,
    found by marking it in the frame and transforming the marks back."""
    s = p.scale
    mark = torch.zeros(1, 1, p.H * s, p.W * s, dtype=torch.bool)
    r0, r1, c0, c1 = p.owned_hr(t)
    mark[:, :, r0:r1, c0:c1] = True
    ys, xs = TR.inverse(mark, k)[0, 0].nonzero(as_tuple=True)
    y, x, hh, ww = int(ys.min()), int(xs.min()), int(ys.max() - ys.min()) + 1, int(xs.max() - xs.min()) + 1
    assert hh * ww == ys.numel()
    return y, x, hh, ww


def _table(A, ents):
    L = A._lib
    descs = []
    for k, p, t in ents:
        oy, ox, oh, ow = _owned_in_image(k, p, t)
        descs.append(L.TileDesc(y0=t.y0, x0=t.x0, id=k, oy=oy, ox=ox, oh=oh, ow=ow, pad_=0))
    host = (L.TileDesc * len(descs))(*descs)
    return host, torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()


def _subsets(n):
    """n in {1, an odd count, all}: (first, count)."""
    odd = min(n, 7) if min(n, 7) % 2 else min(n, 7) - 1
    return sorted({(0, 1), (n - odd, odd), (0, n)})


@pytest.mark.parametrize("h,w", [(45, 59), (20, 59)])
@pytest.mark.parametrize("pad", [8, 0])
@pytest.mark.parametrize("c", [1, 3])
def test_gather_is_torch_indexing(A, h, w, pad, c):
    x = torch.rand(1, c, h, w, generator=torch.Generator().manual_seed(h + pad + c))
    xd = x.cuda()
    ents = _entries(A, h, w, 1, pad)
    for transposed in (False, True):                         # the two tile shapes: a launch holds one
        grp = [e for e in ents if bool(e[0] & 4) == transposed]
        th, tw = grp[0][1].th, grp[0][1].tw
        assert (th, tw) == ((min(w, TILE), min(h, TILE)) if transposed else (min(h, TILE), min(w, TILE)))
        _, table = _table(A, grp)
        want = torch.cat([TR.transform(x, k)[:, :, t.y0:t.y0 + th, t.x0:t.x0 + tw] for k, _, t in grp])
        for first, n in _subsets(len(grp)):
            got = A.tiling.gather(xd, table, first, n, th, tw)
            torch.cuda.synchronize()
            assert tuple(got.shape) == (n, c, th, tw)
            assert torch.equal(got.cpu(), want[first:first + n]), f"{h}x{w} pad {pad} C {c} transposed {transposed} entries {first}+{n}"


@pytest.mark.parametrize("h,w", [(45, 59), (20, 59)])
@pytest.mark.parametrize("pad", [8, 0])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_place_is_torch_indexing(A, h, w, pad, c, scale):
    g = torch.Generator().manual_seed(h + pad + c + scale)
    ents = _entries(A, h, w, scale, pad)
    acc = torch.rand(1, c, h * scale, w * scale, generator=g)           # the accumulate mode's running image
    acc_d = acc.cuda()
    for k in range(8):
        grp = [e for e in ents if e[0] == k]
        p = grp[0][1]
        th, tw, n_all = p.th, p.tw, len(grp)
        host, table = _table(A, grp)
        y = torch.rand(n_all, c, th * scale, tw * scale, generator=g)
        yd = y.cuda()

        def expected(first, n):
            """NaN where nothing is written; the frame is filled from the owned rectangles, then transformed back."""
            frame = torch.full((1, c, p.H * scale, p.W * scale), float("nan"))
            for i in range(first, first + n):
                t = grp[i][2]
                r0, r1, c0, c1 = p.owned_hr(t)
                frame[0, :, r0:r1, c0:c1] = y[i, :, r0 - t.y0 * scale:r1 - t.y0 * scale, c0 - t.x0 * scale:c1 - t.x0 * scale]
            return TR.inverse(frame, k).contiguous()

        for first, n in _subsets(n_all):
            out = torch.full((1, c, h * scale, w * scale), float("nan"), device="cuda")
            ent = host[first:first + n]
            A.tiling.place(yd[first:first + n], out, table, first, n, (h, w), th, tw, scale, max(e.oh for e in ent), max(e.ow for e in ent))
            torch.cuda.synchronize()
            want, got = expected(first, n), out.cpu()
            what = f"{h}x{w} pad {pad} C {c} x{scale} id {k} entries {first}+{n}"
            assert torch.equal(torch.isnan(got), torch.isnan(want)), what + ": another set of pixels was written"
            assert torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0)), what
            if n == n_all:
                assert not bool(torch.isnan(got).any()), what + ": the whole plan leaves pixels unwritten"
        # accumulate, in the order k = 0..7 on one image
        A.tiling.place(yd, acc_d, table, 0, n_all, (h, w), th, tw, scale, max(e.oh for e in host), max(e.ow for e in host), weight=0.125)
        torch.cuda.synchronize()
        acc = acc + 0.125 * expected(0, n_all)
        assert torch.equal(acc_d.cpu(), acc), f"{h}x{w} pad {pad} C {c} x{scale}: accumulate differs after id {k}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------------------
_SMALL = dict(n_feats=64, n_resblocks=2, res_scale=0.1)                 # the small EDSR of eval_ref (OVERFLOW's)
_RCAN = dict(n_feats=64, n_resgroups=2, n_resblocks=3, reduction=16, scale_factor=4)      # eval_ref's small RCAN
MODELS = [
    ER.Case("tiled_edsr_x2", "EDSR", dict(_SMALL, scale_factor=2), H, W, val=True),
    ER.Case("tiled_edsr_x3", "EDSR", dict(_SMALL, scale_factor=3), H, W),
    ER.Case("tiled_edsr_x4", "EDSR", dict(_SMALL, scale_factor=4), H, W, val=True),
    ER.Case("tiled_edsr_gray_x4", "EDSR", dict(n_feats=64, n_resblocks=4, res_scale=1, scale_factor=4, channels=1), H, W, val=True),
    ER.Case("tiled_rdn_a_x4", "RDN", dict(rdn_config="A", scale_factor=4), H, W),
    ER.Case("tiled_wdsr_b_x4", "WDSR", dict(type="B", n_resblocks=4, scale_factor=4), H, W, val=True),
    ER.Case("tiled_srresnet_x2", "SRResNet", dict(n_feats=64, n_resblocks=4, scale_factor=2), H, W),
    ER.Case("tiled_ddbpn_x2", "DDBPN", dict(scale_factor=2), H, W),
    ER.Case("tiled_rcan_x4", "RCAN", _RCAN, H, W, val=True),
]
ENSEMBLE = ER.Case("ens_edsr_x2", "EDSR", dict(_SMALL, scale_factor=2), H, W, val=True)
MODES = ["32", "16", "bf16-storage"]
_DT = {"32": torch.float32, "16": torch.float16, "bf16-storage": torch.bfloat16}


class TiledRef(ER.Ref):
    """eval_ref.Ref with the independent float64 statement of tiling / self-ensemble wrapped around every oracle run."""

    def __init__(self, case, sd, x, tile, pad, ens):
        self.case, self.sd, self.x, self.opts = case, sd, x, (tile, pad, ens)
        raw = self._run(None)
        self.raw_max = float(raw.abs().max())
        self.ref = raw.clamp(0, 1)
        self.base = {}

    def _run(self, dt):
        # the operands are rounded to `dt` inside ER.oracle, per call: rounding commutes with cutting and flipping
        tile, pad, ens = self.opts
        return TR.forward(lambda t: ER.oracle(self.case, self.sd, t, dt), self.x, self.case.scale, tile, pad, ens)

    def baseline(self, dt):
        if dt == torch.float32 and dt not in self.base:
            self.base[dt] = dict(self.baseline(torch.float16), psnr=300.0, u8max=0, u8share=0.0)
        if dt not in self.base:
            y = self._run(dt).clamp(0, 1)
            row, col, peak = ER.local_stats(y - self.ref)
            u8max, u8share = ER.u8_diff(y, self.ref)
            self.base[dt] = dict(row=row, col=col, peak=peak, psnr=ER.psnr_db(y, self.ref), u8max=u8max, u8share=u8share)
        return self.base[dt]


@pytest.fixture(scope="module")
def refs(A):
    """(case id, tile, pad, ensemble) -> TiledRef, computed once and shared by the storage dtypes."""
    cache = {}

    def get(case, tile, pad, ens):
        key = (case.id, tile, pad, ens)
        if key not in cache:
            sd = ER.state_of(ER.new_model(A, case))
            cache[key] = TiledRef(case, sd, ER.image(case.channels, case.h, case.w, ER.case_seed(case)), tile, pad, ens)
        return cache[key]
    get.cache = cache
    return get


def _model(A, ref, mode, **opts):
    extra = dict(eval_precision="bf16") if mode == "bf16-storage" else {}
    m = ER.new_model(A, ref.case, ER.PREC[_DT[mode]], **extra, **opts)
    m.load_state_dict(ref.sd)
    return m.cuda().eval()


def _judge(A, ref, mode, what, **opts):
    m = _model(A, ref, mode, **opts)
    assert m.eval_dtype == _DT[mode]
    y = ER.predict(m, ref.x)
    # bf16 storage at its 50 dB floor cannot hold the uint8 contract (eval_ref.py docstring)
    ER.check_image(y, ref, m.eval_dtype, f"{ref.case.id} {what} precision={mode}")
    assert torch.equal(ER.predict(m, ref.x), y), f"{ref.case.id} {what} {mode}: two runs of one input differ"
    if ref.case.val:
        ER.compare_validation(m, ref, y)
    return m, y


@pytest.mark.parametrize("case", MODELS, ids=lambda c: c.id)
@pytest.mark.parametrize("mode", MODES)
def test_tiled_predict_vs_float64_statement(A, refs, case, mode):
    ref = refs(case, TILE, PAD, False)
    try:
        _judge(A, ref, mode, "tiled", tile=TILE, tile_pad=PAD, tile_batch=BATCH)
    finally:
        if mode == MODES[-1]:
            refs.cache.pop((case.id, TILE, PAD, False), None)


def test_rcan_tiled_is_not_the_whole_image(A, refs):
    """Channel attention pools over the tile: RCAN's tiled image is well defined (the test above) but another one than the whole image's.
    For a convolutional net of radius <= pad the two agree (tests/test_tiling_cpu.py)."""
    case = MODELS[-1]
    sd = ER.state_of(ER.new_model(A, case))
    x = ER.image(case.channels, case.h, case.w, ER.case_seed(case))
    whole = ER.oracle(case, sd, x)
    tiled = TR.forward(lambda t: ER.oracle(case, sd, t), x, case.scale, TILE, PAD)
    assert float((whole - tiled).abs().max()) > 1e-6 * max(1.0, float(whole.abs().max()))


@pytest.mark.parametrize("tile", [0, TILE], ids=["alone", "tiled"])
@pytest.mark.parametrize("mode", MODES)
def test_self_ensemble_vs_float64_statement(A, refs, tile, mode):
    ref = refs(ENSEMBLE, tile, PAD if tile else 0, True)
    opts = dict(tile=tile, tile_pad=PAD, tile_batch=BATCH) if tile else {}
    _judge(A, ref, mode, f"self-ensemble tile={tile}", self_ensemble=True, **opts)


@pytest.mark.parametrize("mode", ["32", "16", "bf16", "bf16-storage"])
def test_off_means_off(A, mode):
    """tile=0, self_ensemble=False: the image of the parent path -- the forward in the evaluation dtype, clamped -- bit for bit, and
    tiling.tiled_forward is not entered."""
    case = ENSEMBLE
    dt = {"bf16": torch.bfloat16}.get(mode) or _DT[mode]
    extra = dict(eval_precision="bf16") if mode == "bf16-storage" else {}
    m = ER.new_model(A, case, ER.PREC[dt], tile=0, self_ensemble=False, **extra).cuda().eval()
    x = ER.image(case.channels, case.h, case.w, ER.case_seed(case)).cuda()
    real = A.tiling.tiled_forward

    def never(*a, **k):
        raise AssertionError("tiled_forward entered with both options off")
    A.tiling.tiled_forward = never
    try:
        with torch.no_grad():
            y = m.predict_step({"lr": x}, 0)
            prev, m.compute_dtype = m.compute_dtype, m.eval_dtype          # the parent's _eval_forward, spelled out
            try:
                want = m.forward(x)
            finally:
                m.compute_dtype = prev
    finally:
        A.tiling.tiled_forward = real
    assert bool(torch.isfinite(want).all())
    assert torch.equal(y, want.clamp(0, 1))
    # and the options change the image (so the comparison above is of the path that is off)
    on = ER.new_model(A, case, ER.PREC[dt], tile=TILE, tile_pad=0, **extra)
    on.load_state_dict(m.state_dict())
    assert not torch.equal(ER.predict(on.cuda().eval(), x), y)


def test_fp16_overflow_rule_on_the_assembled_image(A):
    """A bf16 model whose fp16 evaluation overflows (eval_ref.OVERFLOW) returns its training dtype's tiled image."""
    case = ER.OVERFLOW
    sd = ER.state_of(ER.new_model(A, case))
    x = ER.image(3, case.h, case.w, ER.case_seed(case))
    opts = dict(tile=TILE, tile_pad=PAD, tile_batch=BATCH)

    def on_gpu(precision, **extra):
        m = ER.new_model(A, case, precision, **extra, **opts)
        m.load_state_dict(sd)
        return m.cuda().eval()
    m16 = on_gpu(16)
    with torch.no_grad():
        y16 = A.tiling.tiled_forward(m16.forward, x.cuda(), case.scale, tile=TILE, pad=PAD, tile_batch=BATCH)
    assert not bool(torch.isfinite(y16).all()), "the fp16 tiles stayed finite: the case does not reach the fallback"
    y = ER.predict(on_gpu("bf16"), x)
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, ER.predict(on_gpu("bf16", eval_precision="bf16"), x))
