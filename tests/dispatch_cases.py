"""The case bodies of tests/test_gpu_dispatch_sides.py: the kernels srk_conv2d / srk_conv2d_wgrad / srk_unfold_nchw fall back to when a
`*_ok()` predicate refuses a shape or a maintainer sets an A/B knob (SRK_DEBUG=1, tools/ab_knob.sh), each against float64 of the same
16-bit-rounded operands.  The knobs are read once per process, so every knob setting runs in a fresh child:

    python tests/dispatch_cases.py <setting>        -> one line "RESULT {json}"

The child does the comparison itself.  Per case it reports the kernel family that ran (srk_last_kernel(), read after every _lib.call on
the calling thread, so launches made inside backward() are seen too), the name the fallback must have, whether a NaN of the prefilled
output survived, and the worst error as a fraction of its bound.  The setting "none" launches every case with no knob and reports the
names only: the parent (test_gpu_dispatch_sides.py) asserts that a fallback's name differs from it.

Criteria are those of the existing test of the same operation, unchanged (each group names its source).  Two bounds are derived:

* the r*r-pass data gradient through a PixelShuffle (`ps_dgrad`): see its docstring;
* the generic weight gradient (one slab per workgroup, summed in a fixed order): the bound is the project's fp32-accumulation bound of
  test_grouped_matches_per_layer_and_float64 / test_wgrad_1x1_slab_kernel, on both of two runs, and the two runs are equal bit for bit.

This module is a plain helper (no fixtures, no pytest hooks); importing it needs no GPU (tests/test_dispatch_knobs.py reads SETTINGS)."""
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("srk_conv2d", "srk_conv2d_wgrad", "srk_unfold_nchw")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


class Recorder:
    """Wraps sr_amd._lib.call: after every call of an entry that dispatches, notes (entry, srk_last_kernel(), nslabs of a wgrad)."""

    def __init__(self):
        from sr_amd import _lib as L
        self.L, self.real, self.log = L, L.call, []
        self.lib = L.load()

    def __call__(self, name, args, stream):
        self.real(name, args, stream)
        if name in ENTRIES:
            self.log.append((name, self.lib.srk_last_kernel().decode(), int(getattr(args, "nslabs", -1))))

    def __enter__(self):
        self.L.call = self
        return self

    def __exit__(self, *exc):
        self.L.call = self.real

    def take(self):
        log, self.log = self.log, []
        return log


def _names(log, entry):
    return [k for (e, k, _) in log if e == entry]


def _dtname(dt):
    import torch
    return "bf16" if dt == torch.bfloat16 else "f16"


def _dts():
    import torch
    return [torch.bfloat16, torch.float16]


def _rnd(g, *shape, scale=1.0):
    import torch
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _igemm(coutp, ks):
    return f"conv_igemm<{128 if coutp % 128 == 0 else 64 if coutp % 64 == 0 else 32},{ks}>"


def _case(kernels, expect, nan, ratio=None, why_same=None, **more):
    """kernels / expect: role -> name.  ratio: worst |err| / bound over the case's comparisons (<= 1 passes); None: names only."""
    d = dict(kernels=kernels, expect=expect, nan=bool(nan), ratio=None if ratio is None else float(ratio))
    if why_same:
        d["same_side_because"] = why_same       # the knob cannot move this case: the name must still be `expect`, but equals the no-knob name
    d.update(more)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_raw 3x3 with every epilogue of the weight-stationary kernel -- criterion: test_gpu_ws_epilogue.py::test_ws_epilogue_variants
# ---------------------------------------------------------------------------------------------------------------------------------
WS_VARIANTS = ["plain", "relu", "res", "res_scale", "mask0", "mask16", "res_mask"]
WS_EARLY_VARIANTS = ["res", "res_scale", "mask0", "mask16"]


def ws_epilogue(R, setting, check, variants):
    import torch
    import torch.nn.functional as F
    import sr_amd as A
    out_cases = {}
    for dt in _dts():
        for (cin, cout) in [(64, 64), (16, 64), (64, 3)]:
            for (n, h, w) in [(1, 17, 50), (3, 5, 3)]:
                for variant in variants:
                    g = torch.Generator().manual_seed(_seed(cin, cout, n, h, w, variant))
                    cs = (cout + 15) // 16 * 16                                      # stored channels
                    x = ((torch.rand(n, h, w, cin, generator=g) - 0.5) * 2).to(dt).cuda()
                    wt = ((torch.rand(cout, cin, 3, 3, generator=g) - 0.5) * (2.0 / (cin * 9) ** 0.5)).cuda()
                    b = ((torch.rand(cout, generator=g) - 0.5) * 0.2).cuda()
                    res = ((torch.rand(n, h, w, cs, generator=g) - 0.5) * 2).to(dt).cuda() if "res" in variant else None
                    mask = torch.relu((torch.rand(n, h, w, cs, generator=g) - 0.5)).to(dt).cuda() if "mask" in variant else None
                    mask_from = 16 if variant == "mask16" else 0
                    relu = variant == "relu"
                    scale = 0.1 if variant == "res_scale" else 1.0
                    pk = A.ops.pack_conv(torch.nn.Parameter(wt), torch.nn.Parameter(b), dt)
                    out = torch.full((n, h, w, cs), float("nan"), dtype=dt, device="cuda")
                    R.take()
                    A.ops.conv_raw(x, pk, N=n, H=h, W=w, Cin=cin, Cout=cs, out=out, relu=relu, scale=scale, res=res, mask=mask, mask_from=mask_from)
                    torch.cuda.synchronize()
                    kern = {"fwd": _names(R.take(), "srk_conv2d")[-1]}
                    why = None
                    if setting == "SRK_NO_WS":
                        expect = {"fwd": _igemm(pk.CoutP, 3)}
                    elif setting == "SRK_NO_EARLY":
                        expect = {"fwd": "conv_ws<1,4,0,0>" if cout == 3 else f"conv_ws<2,{4 if cin == 64 else 1},0,0>"}
                        if cout == 3:
                            why = "the 32-row kernel (64 -> 3) has no prefetch variant"
                    else:
                        expect = {}
                    cid = f"ws_epilogue/{_dtname(dt)}/{cin}to{cout}/{n}x{h}x{w}/{variant}"
                    nan = not bool(torch.isfinite(out.float()).all())
                    if not check:
                        out_cases[cid] = _case(kern, expect, nan)
                        continue
                    wq = wt.to(dt).double().cpu()
                    ref = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), wq, b.double().cpu(), padding=1).permute(0, 2, 3, 1)
                    if relu:
                        ref = ref.clamp_min(0)
                    ref = ref * scale
                    zeros_ok = True
                    if res is not None:
                        ref = ref + res.double().cpu()[..., :cout]
                    if mask is not None:
                        keep = mask.double().cpu()[..., :cout] > 0
                        keep[..., :mask_from] = True
                        ref = torch.where(keep, ref, torch.zeros_like(ref))
                        zeros_ok = bool((out.cpu()[..., :cout][~keep] == 0).all())      # masked elements are exactly zero
                    got = out.double().cpu()[..., :cout]
                    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
                    err = (got - ref).abs()
                    tol = eps * ref.abs() * 1.5 + 4e-3 * eps * 256 / 256 + 1e-3 * float(ref.abs().max()) * (1 if dt == torch.bfloat16 else 0.1)
                    ratio = float((err / tol).max()) if zeros_ok else float("inf")
                    out_cases[cid] = _case(kern, expect, nan, ratio, why, err=float(err.max()), masked_zeros_exact=zeros_ok)
    return out_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# wgrad_raw, the generic kernel -- criteria: test_gpu_wgrad_group.py::test_grouped_matches_per_layer_and_float64 (3x3: 1e-4 of the largest
# entry) and test_gpu_ws_epilogue.py::test_wgrad_1x1_slab_kernel (1x1: 2e-5 * max(1, largest entry)); two runs, both bounded, and equal
# bit for bit (`run_to_run`: the largest difference, NaN-proof through the integer view)
# ---------------------------------------------------------------------------------------------------------------------------------
def generic_slabs(n, h, w, cin, cout):
    """The generic kernel's grid over 16 x 16 pixel tiles and 64-channel blocks (16-bit): one slab per blockIdx.x."""
    tiles = n * ((h + 15) // 16) * ((w + 15) // 16)
    return max(1, min(tiles, 256 // (((cin + 63) // 64) * ((cout + 63) // 64))))


def wgrad_generic(R, setting, check):
    import torch
    import sr_amd as A
    out_cases = {}
    shapes = [(3, 2, 17, 20, 64, 64), (3, 1, 5, 3, 64, 16), (3, 2, 9, 31, 128, 64), (3, 1, 16, 16, 64, 256),
              (1, 2, 13, 7, 128, 768), (1, 2, 13, 7, 576, 64), (1, 1, 1, 1, 64, 64)]
    for dt in _dts():
        for (k, n, h, w, cin, cout) in shapes:
            g = torch.Generator().manual_seed(_seed("wgrad", k, n, h, w, cin, cout))
            amp = 1.0 if k == 3 else 2.0                      # the operand ranges of the two source tests
            x = ((torch.rand(n, h, w, cin, generator=g) - 0.5) * amp).to(dt).cuda()
            dy = ((torch.rand(n, h, w, cout, generator=g) - 0.5) * amp).to(dt).cuda()
            runs, kerns, slabs, nan = [], [], [], False
            for _ in range(2):
                dw = torch.full((cout, cin, k, k), float("nan"), device="cuda")
                db = torch.full((cout,), float("nan"), device="cuda")
                R.take()
                A.ops.wgrad_raw(x, dy, N=n, H=h, W=w, Cin=cin, Cout=cout, k=k, w_shape=(cout, cin, k, k), out_w=dw, out_b=db)
                torch.cuda.synchronize()
                log = [t for t in R.take() if t[0] == "srk_conv2d_wgrad"]
                kerns.append(log[-1][1])
                slabs.append(log[-1][2])
                nan = nan or not bool(torch.isfinite(dw).all() and torch.isfinite(db).all())
                runs.append((dw.double().cpu(), db.double().cpu(), dw.view(torch.int32).cpu(), db.view(torch.int32).cpu()))
            kern = {"wgrad": kerns[0], "wgrad_second_run": kerns[1]}
            expect = {"wgrad": f"wgrad_generic<{k}>", "wgrad_second_run": f"wgrad_generic<{k}>"} if setting == "SRK_NO_WS" else {}
            cid = f"wgrad_generic/{_dtname(dt)}/k{k}/{n}x{h}x{w}/{cin}to{cout}"
            if not check:
                out_cases[cid] = _case(kern, expect, nan, nslabs=slabs)
                continue
            want_slabs = generic_slabs(n, h, w, cin, cout)
            ref_w = torch.nn.grad.conv2d_weight(x.double().cpu().permute(0, 3, 1, 2), (cout, cin, k, k), dy.double().cpu().permute(0, 3, 1, 2), padding=k // 2)
            ref_b = dy.double().cpu().sum((0, 1, 2))
            if k == 3:
                tw, tb = 1e-4 * float(ref_w.abs().max()), 1e-4 * float(ref_b.abs().max())
            else:
                tw, tb = 2e-5 * max(1.0, float(ref_w.abs().max())), 2e-5 * max(1.0, float(ref_b.abs().max()))
            ratio = max(max(float((dw - ref_w).abs().max()) / tw, float((db - ref_b).abs().max()) / tb) for (dw, db, _, _) in runs)
            same = torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])
            out_cases[cid] = _case(kern, expect, nan, ratio, nslabs=slabs, nslabs_generic=[want_slabs, want_slabs], bitwise_repeat=bool(same),
                                   run_to_run=float((runs[0][0] - runs[1][0]).abs().max()))
    return out_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# the streaming 3x3 kernel on conv_ks's shapes -- criteria: tests/test_gpu_conv_ks.py (the five forms, the channel slices, the fused
# PixelShuffle store with the data gradient read through it)
# ---------------------------------------------------------------------------------------------------------------------------------
KS_SHAPES = [(2, 20, 33, 128, 64), (1, 7, 9, 512, 128), (1, 1, 1, 128, 64), (2, 17, 31, 256, 192)]


def ks_forms(R, setting, check):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import sr_amd as A
    dev = torch.device("cuda")
    out_cases = {}
    for dt in _dts():
        for form in ["bias_relu", "scale_res", "mask", "res_mask_from", "dgrad_mask"]:
            for (n, h, w, ci, co) in KS_SHAPES:
                g = torch.Generator().manual_seed(_seed("ks", form, n, h, w, ci, co))
                x = _rnd(g, n, h, w, ci).to(dt)
                wt = _rnd(g, co, ci, 3, 3, scale=1.0 / np.sqrt(9 * ci))
                b = _rnd(g, co, scale=0.2)
                res = _rnd(g, n, h, w, co).to(dt)
                mk = torch.relu(_rnd(g, n, h, w, co)).to(dt)
                dgrad = form == "dgrad_mask"
                wp, bp = torch.nn.Parameter(wt.to(dev)), torch.nn.Parameter(b.to(dev))
                kw = dict(relu=False, scale=1.0, res=None, mask=None, mask_from=0, use_bias=not dgrad)
                if dgrad:
                    wt2 = _rnd(g, ci, co, 3, 3, scale=1.0 / np.sqrt(9 * ci))
                    wp = torch.nn.Parameter(wt2.to(dev))
                    pk = A.ops.pack_conv(wp, None, dt, dgrad=True)
                    kw.update(mask=mk.to(dev))
                else:
                    pk = A.ops.pack_conv(wp, bp, dt)
                    if form == "bias_relu":
                        kw.update(relu=True)
                    elif form == "scale_res":
                        kw.update(scale=0.1, res=res.to(dev))
                    elif form == "mask":
                        kw.update(mask=mk.to(dev))
                    else:
                        kw.update(res=res.to(dev), mask=mk.to(dev), mask_from=32 if co > 32 else 0)
                out = torch.full((n, h, w, co), float("nan"), dtype=dt, device=dev)
                R.take()
                A.ops.conv_raw(x.to(dev), pk, N=n, H=h, W=w, Cin=ci, Cout=co, out=out, **kw)
                torch.cuda.synchronize()
                kern = {"fwd": _names(R.take(), "srk_conv2d")[-1]}
                expect = {"fwd": _igemm(pk.CoutP, 3)} if setting == "SRK_NO_KS" else {}
                cid = f"ks_forms/{_dtname(dt)}/{form}/{n}x{h}x{w}/{ci}to{co}"
                got = out.double().cpu().permute(0, 3, 1, 2)
                nan = not bool(torch.isfinite(got).all())
                if not check:
                    out_cases[cid] = _case(kern, expect, nan)
                    continue
                if dgrad:
                    ref = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), wt2.to(dt).double(), padding=1)
                    ref = torch.where(mk.double().permute(0, 3, 1, 2) > 0, ref, torch.zeros_like(ref))
                else:
                    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.to(dt).double(), b.double(), padding=1)
                    if form == "bias_relu":
                        ref = torch.relu(ref)
                    elif form == "scale_res":
                        ref = ref * 0.1 + res.double().permute(0, 3, 1, 2)
                    elif form == "mask":
                        ref = torch.where(mk.double().permute(0, 3, 1, 2) > 0, ref, torch.zeros_like(ref))
                    else:
                        mf = 32 if co > 32 else 0
                        ref = ref + res.double().permute(0, 3, 1, 2)
                        m = mk.double().permute(0, 3, 1, 2) > 0
                        m[:, :mf] = True
                        ref = torch.where(m, ref, torch.zeros_like(ref))
                tol = (2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10) * max(1.0, float(ref.abs().max()))
                err = float((got - ref).abs().max())
                out_cases[cid] = _case(kern, expect, nan, err / tol, err=err)
    return out_cases


def ks_slices(R, setting, check):
    """test_conv_ks_on_channel_slices: the conv reads the first 128 / 192 channels of a wider buffer and writes a 64-channel slice of it."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import sr_amd as A
    dev, dt = torch.device("cuda"), torch.bfloat16
    g = torch.Generator().manual_seed(3)
    n, h, w = 2, 19, 30
    feat = _rnd(g, n, h, w, 320).to(dt).to(dev)
    ref_feat = feat.clone()
    out_cases = {}
    for cin in (128, 192):
        wt = _rnd(g, 64, cin, 3, 3, scale=1.0 / np.sqrt(9 * cin))
        b = _rnd(g, 64, scale=0.2)
        pk = A.ops.pack_conv(torch.nn.Parameter(wt.to(dev)), torch.nn.Parameter(b.to(dev)), dt)
        feat[..., cin:cin + 64] = float("nan")
        R.take()
        A.ops.conv_raw(feat[..., :cin], pk, N=n, H=h, W=w, Cin=cin, Cout=64, out=feat[..., cin:cin + 64], relu=True)
        torch.cuda.synchronize()
        kern = {"fwd": _names(R.take(), "srk_conv2d")[-1]}
        expect = {"fwd": "conv_igemm<64,3>"} if setting == "SRK_NO_KS" else {}
        got = feat[..., cin:cin + 64].double().cpu().permute(0, 3, 1, 2)
        nan = not bool(torch.isfinite(got).all())
        cid = f"ks_slices/bf16/{cin}"
        if check:
            r = torch.relu(F.conv2d(ref_feat[..., :cin].double().cpu().permute(0, 3, 1, 2), wt.to(dt).double(), b.double(), padding=1))
            err = float((got - r).abs().max())
            same = torch.equal(feat[..., cin + 64:], ref_feat[..., cin + 64:]) and torch.equal(feat[..., :cin], ref_feat[..., :cin])      # the channels beside the slice
            out_cases[cid] = _case(kern, expect, nan, err / (2.0 ** -7 * max(1.0, float(r.abs().max()))) if same else float("inf"), err=err, neighbours_untouched=same)
        else:
            out_cases[cid] = _case(kern, expect, nan)
        ref_feat = feat.clone()
    return out_cases


def ks_ps_store(R, setting, check):
    """test_conv_ks_pixelshuffle_store_and_shuffled_input: conv 128 -> 512 with the fused PixelShuffle(2) store, and its data gradient."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import sr_amd as A
    dev = torch.device("cuda")
    out_cases = {}
    for dt in _dts():
        g = torch.Generator().manual_seed(17)
        n, h, w, f, r = 2, 11, 13, 128, 2
        x = _rnd(g, n, f, h, w)
        wt = _rnd(g, f * r * r, f, 3, 3, scale=1.0 / np.sqrt(9 * f))
        b = _rnd(g, f * r * r, scale=0.1)
        xq = x.to(dt).double().requires_grad_(True)
        y = F.pixel_shuffle(F.conv2d(xq, wt.to(dt).double(), b.double(), padding=1), r)
        gy = _rnd(g, *y.shape).to(dt).double()
        xd = x.permute(0, 2, 3, 1).contiguous().to(dt).to(dev).requires_grad_(True)
        wp, bp = torch.nn.Parameter(wt.to(dev)), torch.nn.Parameter(b.to(dev))
        R.take()
        yd = A.ops.conv(xd, wp, bp, ps_r=r)
        yd.backward(gy.permute(0, 2, 3, 1).contiguous().to(dt).to(dev))
        torch.cuda.synchronize()
        names = _names(R.take(), "srk_conv2d")
        kern = {"fwd": names[0], "dgrad": names[1]}
        expect = {"fwd": "conv_igemm<128,3>", "dgrad": "conv_igemm<128,3>"} if setting == "SRK_NO_KS" else {}
        got = yd.detach().double().cpu().permute(0, 3, 1, 2)
        gx = xd.grad.double().cpu().permute(0, 3, 1, 2)
        nan = not bool(torch.isfinite(got).all() and torch.isfinite(gx).all())
        cid = f"ks_ps_store/{_dtname(dt)}"
        if check:
            y.backward(gy)
            tol = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
            e1 = float((got - y.detach()).abs().max()) / (tol * max(1.0, float(y.abs().max())))
            e2 = float((gx - xq.grad).abs().max()) / (2 * tol * max(1.0, float(xq.grad.abs().max())))
            out_cases[cid] = _case(kern, expect, nan, max(e1, e2), fwd_ratio=e1, dgrad_ratio=e2)
        else:
            out_cases[cid] = _case(kern, expect, nan)
    return out_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# the r*r-pass weight-stationary data gradient through a PixelShuffle (launch_ws with x_ps > 1) -- derived bound
# ---------------------------------------------------------------------------------------------------------------------------------
def ps_dgrad(R, setting, check):
    """conv_raw(g, dgrad pack of a 64 -> 64 r^2 upsampler conv, x_ps = r): r = 2 (Cin 256) and r = 3 (Cin 576), alone, with `res`
    (scale 0.5) and with `mask`.

    The kernel runs r*r weight-stationary 64 -> 64 passes, one per sub-pixel (i, j) of the shuffled gradient, in the order
    ij = i*r + j, and keeps the running sum in `out` in the 16-bit storage type:
        pass 0: out = rnd(scale*conv_0 + res);   pass ij > 0: out = rnd(scale*conv_ij + out);   the mask runs with the last pass.
    The float64 reference forms the same partial sums S_0 .. S_{r*r-1} in that order and rounds to the storage type after each.  Every
    pass is one launch of the kernel test_ws_epilogue_variants bounds to one rounding,
        |got - ref| <= 1.5*eps*|ref| + 4e-3*eps + 1e-3*max|ref| * (1 for bf16, 0.1 for fp16),
    and a deviation of the running sum carried into the next pass is at most re-rounded there, which that pass's bound covers; so after
    r*r passes the result is within r*r times that bound, taken against the largest partial sum: per element P = max_k |S_k| in the
    relative term, the largest |S_k| of the whole tensor in the last.  Masked elements are exactly zero.

    (What these rows can and cannot see: a mask applied on an earlier pass only, a residual added on a later pass, a wrong weight slab or
    sub-pixel offset all change the numbers.  A mask applied on EVERY pass does not -- a masked element is then zero after each pass
    instead of after the last, every other element is untouched -- so that variation passes, as it should.)"""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import sr_amd as A
    dev = torch.device("cuda")
    out_cases = {}
    for dt in _dts():
        for r in (2, 3):
            r2, cin = r * r, 64 * r * r
            for (n, h, w) in [(2, 11, 13), (3, 5, 3), (1, 1, 1)]:
                for variant in ("alone", "res", "mask"):
                    g = torch.Generator().manual_seed(_seed("psd", r, n, h, w, variant))
                    wt = _rnd(g, cin, 64, 3, 3, scale=1.0 / np.sqrt(9 * cin))                       # the upsampler conv 64 -> 64 r^2 (torch channel order c*r2 + ij)
                    gy = _rnd(g, n, 64, h * r, w * r).to(dt)                                       # gradient of the shuffled output
                    res = _rnd(g, n, h, w, 64).to(dt) if variant == "res" else None
                    mk = torch.relu(_rnd(g, n, h, w, 64)).to(dt) if variant == "mask" else None
                    scale = 0.5 if variant == "res" else 1.0
                    pkd = A.ops.pack_conv(torch.nn.Parameter(wt.to(dev)), None, dt, dgrad=True, ps_r=r)
                    gx = torch.full((n, h, w, 64), float("nan"), dtype=dt, device=dev)
                    R.take()
                    A.ops.conv_raw(gy.permute(0, 2, 3, 1).contiguous().to(dev), pkd, N=n, H=h, W=w, Cin=cin, Cout=64, out=gx, scale=scale, x_ps=r,
                                   use_bias=False, res=None if res is None else res.to(dev), mask=None if mk is None else mk.to(dev))
                    torch.cuda.synchronize()
                    kern = {"dgrad": _names(R.take(), "srk_conv2d")[-1]}
                    # the name is the last pass's: its residual is `out` (the prefetch variant); with a mask too, the plain variant
                    last = "0,0" if variant == "mask" else "1,1"
                    expect = {"dgrad": f"conv_ws<2,4,{last}>x{r2}"} if setting in ("SRK_NO_KS", "SRK_PS_DGRAD_WS") else {}
                    cid = f"ps_dgrad/{_dtname(dt)}/r{r}/{n}x{h}x{w}/{variant}"
                    got = gx.double().cpu().permute(0, 3, 1, 2)
                    nan = not bool(torch.isfinite(got).all())
                    if not check:
                        out_cases[cid] = _case(kern, expect, nan)
                        continue
                    gyu = F.pixel_unshuffle(gy.double(), r)                                     # [n, c*r2 + ij, h, w]
                    wq = wt.to(dt).double()
                    acc = None if res is None else res.double().permute(0, 3, 1, 2)
                    pmax = torch.zeros(n, 64, h, w, dtype=torch.float64)
                    for ij in range(r2):
                        part = scale * F.conv_transpose2d(gyu[:, ij::r2], wq[ij::r2], padding=1)
                        acc = (part if acc is None else part + acc).to(dt).double()                # the running sum lives in the storage type
                        pmax = torch.maximum(pmax, acc.abs())
                    zeros_ok = True
                    if mk is not None:
                        keep = mk.double().permute(0, 3, 1, 2) > 0
                        acc = torch.where(keep, acc, torch.zeros_like(acc))
                        zeros_ok = bool((got[~keep] == 0).all())
                    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
                    tol = r2 * (eps * pmax * 1.5 + 4e-3 * eps + 1e-3 * float(pmax.max()) * (1 if dt == torch.bfloat16 else 0.1))
                    err = (got - acc).abs()
                    ratio = float((err / tol).max()) if zeros_ok else float("inf")
                    out_cases[cid] = _case(kern, expect, nan, ratio, err=float(err.max()), masked_zeros_exact=zeros_ok, largest_partial_sum=float(pmax.max()))
    return out_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# the streaming 1x1 kernel on conv1x1's shapes -- criterion: tests/test_gpu_conv_ks.py::test_conv1x1_against_float64
# ---------------------------------------------------------------------------------------------------------------------------------
def p1_forms(R, setting, check):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import sr_amd as A
    dev = torch.device("cuda")
    out_cases = {}
    for dt in _dts():
        for form in ["bias_relu", "scale_res", "mask", "res_mask_from"]:
            for ci in (64, 256, 576):
                for (n, h, w) in [(2, 13, 7), (1, 1, 1)]:
                    co = 64
                    g = torch.Generator().manual_seed(_seed("p1", form, ci, n, h, w))
                    x = _rnd(g, n, h, w, ci).to(dt)
                    wt = _rnd(g, co, ci, 1, 1, scale=1.0 / np.sqrt(ci))
                    b = _rnd(g, co, scale=0.2)
                    res = _rnd(g, n, h, w, co).to(dt)
                    mk = torch.relu(_rnd(g, n, h, w, co)).to(dt)
                    pk = A.ops.pack_conv(torch.nn.Parameter(wt.to(dev)), torch.nn.Parameter(b.to(dev)), dt)
                    kw = dict(relu=False, scale=1.0, res=None, mask=None, mask_from=0)
                    if form == "bias_relu":
                        kw.update(relu=True)
                    elif form == "scale_res":
                        kw.update(scale=0.3, res=res.to(dev))
                    elif form == "mask":
                        kw.update(mask=mk.to(dev))
                    else:
                        kw.update(res=res.to(dev), mask=mk.to(dev), mask_from=32)
                    out = torch.full((n, h, w, co), float("nan"), dtype=dt, device=dev)
                    R.take()
                    A.ops.conv_raw(x.to(dev), pk, N=n, H=h, W=w, Cin=ci, Cout=co, out=out, **kw)
                    torch.cuda.synchronize()
                    kern = {"fwd": _names(R.take(), "srk_conv2d")[-1]}
                    expect = {"fwd": "conv_igemm<64,1>"} if setting == "SRK_NO_P1" else {}
                    cid = f"p1_forms/{_dtname(dt)}/{form}/{ci}to{co}/{n}x{h}x{w}"
                    got = out.double().cpu().permute(0, 3, 1, 2)
                    nan = not bool(torch.isfinite(got).all())
                    if not check:
                        out_cases[cid] = _case(kern, expect, nan)
                        continue
                    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.to(dt).double(), b.double())
                    resr, mkr = res.double().permute(0, 3, 1, 2), mk.double().permute(0, 3, 1, 2)
                    if form == "bias_relu":
                        ref = torch.relu(ref)
                    elif form == "scale_res":
                        ref = ref * 0.3 + resr
                    elif form == "mask":
                        ref = torch.where(mkr > 0, ref, torch.zeros_like(ref))
                    else:
                        ref = ref + resr
                        m = mkr > 0
                        m[:, :32] = True
                        ref = torch.where(m, ref, torch.zeros_like(ref))
                    tol = (2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10) * max(1.0, float(ref.abs().max()))
                    err = float((got - ref).abs().max())
                    out_cases[cid] = _case(kern, expect, nan, err / tol, err=err)
    return out_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# the collapsed HR stage's forward: 5x5, planar PixelShuffle(2) store, post_add -- criterion:
# tests/test_gpu_conv_lk_elements.py::test_collapsed_stage_forward_kernel_per_element
# ---------------------------------------------------------------------------------------------------------------------------------
COLLAPSED_ALL = [(3, 3, 37, 61), (3, 1, 5, 29), (1, 1, 9, 57), (4, 2, 20, 33)]
COLLAPSED_ROWS = [(3, 3, 37, 61), (3, 1, 5, 29), (1, 1, 9, 57), (2, 2, 16, 28)]


def collapsed_fwd_one(dt, O, n, h, w, seed=None):
    """The body of test_collapsed_stage_forward_kernel_per_element: returns (got, inputs for the reference)."""
    import numpy as np
    import torch
    from sr_amd import ops, _lib as L
    g = torch.Generator().manual_seed(5 + O + h + w if seed is None else seed)
    x = (torch.rand(n, 64, h, w, generator=g) * 2 - 1).to(dt)
    wt = (((torch.rand(4 * O, 64, 5, 5, generator=g) * 2 - 1) / np.sqrt(64 * 25)).to(dt)).float()
    b = (torch.rand(4 * O, generator=g) * 2 - 1) * 0.1
    post = torch.rand(O, generator=g)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    pk = ops.pack_conv(wt.cuda(), b.cuda(), dt, cache=False)
    out = torch.full((n, O, 2 * h, 2 * w), float("nan"), device="cuda")
    ops.conv_raw(xd, pk, N=n, H=h, W=w, Cin=64, Cout=4 * O, out=out, out_mode=L.OUT_PLANAR, ps_r=2, post_add=post.cuda())
    torch.cuda.synchronize()
    return out.cpu().double(), (x, wt, b, post)


def collapsed_ref(x, wt, b, post):
    import torch.nn.functional as F
    return F.pixel_shuffle(F.conv2d(x.double(), wt.double(), b.double(), padding=2), 2) + post.double().view(1, -1, 1, 1)


def collapsed_fwd(R, setting, check, shapes):
    import torch
    out_cases = {}
    for dt in _dts():
        for (O, n, h, w) in shapes:
            R.take()
            got, ins = collapsed_fwd_one(dt, O, n, h, w)
            kern = {"fwd": _names(R.take(), "srk_conv2d")[-1]}
            expect = {"fwd": "lk_conv<8,1,5>"} if setting == "SRK_NO_LK5" else {"fwd": "lk5_fwd"} if setting == "SRK_NO_LK5_ROWS" else {}
            cid = f"collapsed_fwd/{_dtname(dt)}/O{O}/{n}x{h}x{w}"
            nan = not bool(torch.isfinite(got).all())
            if not check:
                out_cases[cid] = _case(kern, expect, nan)
                continue
            ref = collapsed_ref(*ins)
            err = float((got - ref).abs().max())
            out_cases[cid] = _case(kern, expect, nan, err / (2e-5 * float(ref.abs().max())), err=err)
    return out_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# the direct large-kernel convs through autograd: forward, data gradient, weight and bias gradients -- criterion:
# tests/test_gpu_conv_lk_elements.py::test_large_kernel_convs_per_element_on_rounded_inputs
# ---------------------------------------------------------------------------------------------------------------------------------
LK_5X5 = [(5, 12, 3, 48, 48), (5, 8, 1, 21, 19)]
LK_FEW = [(9, 3, 2, 40, 33), (9, 1, 1, 35, 20), (7, 4, 2, 16, 47)]
LK_WGRAD = LK_FEW + [(5, 6, 1, 33, 33)]


def lk_run(R, dt, k, cout, n, h, w):
    """The launches of test_large_kernel_convs_per_element_on_rounded_inputs; returns the outputs, the inputs and the kernel names."""
    import numpy as np
    import torch
    from sr_amd import ops
    g = torch.Generator().manual_seed(17 + k + cout)
    x = (torch.rand(n, 64, h, w, generator=g) * 2 - 1).to(dt)
    wt = (((torch.rand(cout, 64, k, k, generator=g) * 2 - 1) / np.sqrt(64 * k * k)).to(dt)).float()      # weights already representable
    b = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    gy = (torch.rand(n, cout, h, w, generator=g) * 2 - 1).to(dt)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    R.take()
    y = ops.conv_general(xd, wd, bd, stride=1, pad=k // 2)
    cp = y.shape[3]
    gyd = torch.zeros(n, h, w, cp, dtype=dt)
    gyd[..., :cout] = gy.permute(0, 2, 3, 1)
    y.backward(gyd.cuda())
    torch.cuda.synchronize()
    log = R.take()
    convs, wg = _names(log, "srk_conv2d"), _names(log, "srk_conv2d_wgrad")
    assert len(convs) == 2 and len(wg) == 1, log
    return (y, xd.grad, wd.grad, bd.grad), (x, wt, b, gy), {"fwd": convs[0], "dgrad": convs[1], "wgrad": wg[0]}


def lk_ratios(dt, cout, outs, ins):
    """The four comparisons of that test as |err| / bound (each must be <= 1), and whether the padding channels are zero."""
    import torch
    import torch.nn.functional as F
    y, gxd, gwd, gbd = outs
    x, wt, b, gy = ins
    k = wt.shape[2]
    x64, w64, b64 = x.double().requires_grad_(True), wt.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv2d(x64, w64, b64, padding=k // 2)
    ref.backward(gy.double())
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    yy = y.detach().float().cpu()[..., :cout].permute(0, 3, 1, 2).double()
    r = ref.detach()
    gx = gxd.float().cpu().permute(0, 3, 1, 2).double()
    pad_zero = float(y.detach().float()[..., cout:].abs().max()) == 0.0 if y.shape[3] > cout else True
    return dict(fwd=float((yy - r).abs().max()) / (1.1 * eps * float(r.abs().max()) + 1e-6),
                dgrad=float((gx - x64.grad).abs().max()) / (1.1 * eps * float(x64.grad.abs().max()) + 1e-6),
                wgrad=float((gwd.cpu().double() - w64.grad).abs().max()) / (1e-3 * float(w64.grad.abs().max())),
                bgrad=float((gbd.cpu().double() - b64.grad).abs().max()) / (1e-3 * float(b64.grad.abs().max()) + 1e-5)), pad_zero


def _lk_expect(setting, k, cout):
    if setting == "SRK_NO_LK5":
        return {"dgrad": "lk_conv<2,2,5>", "wgrad": "lk_wgrad<5>"}, None
    if setting == "SRK_NO_LK5_DGRAD":
        return {"dgrad": "lk_conv<2,2,5>"}, None
    if setting == "SRK_NO_LK_ROWS":
        return {"fwd": f"lk_conv<8,1,{k}>"}, None
    if setting == "SRK_NO_LK_ALLROWS":
        return {"wgrad": f"lk_wgrad_packed<{k}>"}, ("six output channels are more than the all-rows kernel takes" if cout > 4 else None)
    if setting == "SRK_NO_LK_PACKED":
        return {"wgrad": f"lk_wgrad<{k}>"}, None
    return {}, None


def lk_elements(R, setting, check, shapes):
    import torch
    out_cases = {}
    for dt in _dts():
        for (k, cout, n, h, w) in shapes:
            outs, ins, kern = lk_run(R, dt, k, cout, n, h, w)
            expect, why = _lk_expect(setting, k, cout)
            cid = f"lk_elements/{_dtname(dt)}/k{k}/cout{cout}/{n}x{h}x{w}"
            nan = not all(bool(torch.isfinite(t.float()).all()) for t in outs)
            if not check:
                out_cases[cid] = _case(kern, expect, nan)
                continue
            ratios, pad_zero = lk_ratios(dt, cout, outs, ins)
            out_cases[cid] = _case(kern, expect, nan, max(ratios.values()) if pad_zero else float("inf"), why, ratios=ratios, padding_channels_zero=pad_zero)
    return out_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# srk_unfold_nchw's one-thread-per-pixel kernel at small sizes -- criterion (exact):
# tests/test_gpu_head_conv.py::test_head_unfold_one_thread_per_pixel_is_exact.  Every element of the result is compared, so a
# pixel the kernel never wrote cannot pass (the wrapper allocates the output itself: no prefill).
# ---------------------------------------------------------------------------------------------------------------------------------
def unfold_px(R, setting, check):
    import torch
    import sr_amd as A
    out_cases = {}
    for dtype in _dts():
        for shape in [(1, 3, 1, 1), (2, 3, 5, 7), (1, 3, 17, 50)]:
            torch.manual_seed(11)
            x = torch.rand(*shape).cuda()
            sub = torch.tensor([0.4488, 0.4371, 0.4040], device="cuda")
            R.take()
            got = A.ops.unfold_raw(x, sub, 3, dtype)
            got0 = A.ops.unfold_raw(x, None, 3, dtype)
            torch.cuda.synchronize()
            names = _names(R.take(), "srk_unfold_nchw")
            kern = {"sub": names[0], "plain": names[1]}
            expect = {"sub": "unfold3x3c3", "plain": "unfold3x3c3"} if setting == "SRK_UNFOLD_PX" else {}
            n, c, h, w = shape
            cid = f"unfold_px/{_dtname(dtype)}/{n}x{h}x{w}"
            nan = not bool(torch.isfinite(got.float()).all() and torch.isfinite(got0.float()).all())
            if not check:
                out_cases[cid] = _case(kern, expect, nan)
                continue
            ref = torch.nn.functional.unfold(x - sub.view(1, 3, 1, 1), 3, padding=1).view(n, 27, h, w).permute(0, 2, 3, 1).to(dtype)
            ref0 = torch.nn.functional.unfold(x, 3, padding=1).view(n, 27, h, w).permute(0, 2, 3, 1).to(dtype)
            exact = (got.shape == (n, h, w, 32) and torch.equal(got[..., :27], ref) and not bool(got[..., 27:].any())
                     and torch.equal(got0[..., :27], ref0) and not bool(got0[..., 27:].any()))
            out_cases[cid] = _case(kern, expect, nan, 0.0 if exact else float("inf"), exact=bool(exact))
    return out_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# the knob settings: name -> (environment beside SRK_DEBUG=1, groups, timeout of the child in seconds)
# ---------------------------------------------------------------------------------------------------------------------------------
def _g(fn, **kw):
    return (fn, kw)


SETTINGS = {
    "SRK_NO_WS": ({"SRK_NO_WS": "1"}, [_g(ws_epilogue, variants=WS_VARIANTS), _g(wgrad_generic)], 240),
    "SRK_NO_EARLY": ({"SRK_NO_EARLY": "1"}, [_g(ws_epilogue, variants=WS_EARLY_VARIANTS)], 180),
    "SRK_NO_KS": ({"SRK_NO_KS": "1"}, [_g(ks_forms), _g(ks_slices), _g(ks_ps_store), _g(ps_dgrad)], 300),
    "SRK_PS_DGRAD_WS": ({"SRK_PS_DGRAD_WS": "1"}, [_g(ps_dgrad)], 180),
    "SRK_NO_P1": ({"SRK_NO_P1": "1"}, [_g(p1_forms)], 180),
    "SRK_NO_LK5": ({"SRK_NO_LK5": "1"}, [_g(collapsed_fwd, shapes=COLLAPSED_ALL), _g(lk_elements, shapes=LK_5X5)], 240),
    "SRK_NO_LK5_ROWS": ({"SRK_NO_LK5_ROWS": "1"}, [_g(collapsed_fwd, shapes=COLLAPSED_ROWS)], 180),
    "SRK_NO_LK5_DGRAD": ({"SRK_NO_LK5_DGRAD": "1"}, [_g(lk_elements, shapes=LK_5X5)], 180),
    "SRK_NO_LK_ROWS": ({"SRK_NO_LK_ROWS": "1"}, [_g(lk_elements, shapes=LK_FEW)], 180),
    "SRK_NO_LK_ALLROWS": ({"SRK_NO_LK_ALLROWS": "1"}, [_g(lk_elements, shapes=LK_WGRAD)], 180),
    "SRK_NO_LK_PACKED": ({"SRK_NO_LK_PACKED": "1"}, [_g(lk_elements, shapes=LK_WGRAD)], 180),
    "SRK_UNFOLD_PX": ({"SRK_UNFOLD_PX": "1"}, [_g(unfold_px)], 120),
}
# the no-knob child launches the union of all cases (names only, no float64 work)
NONE_GROUPS = [_g(ws_epilogue, variants=WS_VARIANTS), _g(wgrad_generic), _g(ks_forms), _g(ks_slices), _g(ks_ps_store), _g(ps_dgrad), _g(p1_forms),
               _g(collapsed_fwd, shapes=COLLAPSED_ALL + [s for s in COLLAPSED_ROWS if s not in COLLAPSED_ALL]),
               _g(lk_elements, shapes=LK_5X5 + LK_WGRAD), _g(unfold_px)]
NONE_TIMEOUT = 240
KNOBS = sorted({k for env, _, _ in SETTINGS.values() for k in env})


def child_env(setting):
    """The child's environment: no SRK_* variable of the caller's survives but the library path, then SRK_DEBUG=1 and the setting's knob."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SRK_") or k in ("SRK_LIB_PATH",)}
    if setting != "none":
        env.update(SETTINGS[setting][0], SRK_DEBUG="1")
    return env


def run(setting):
    sys.path.insert(0, ROOT)
    import torch
    import sr_amd as A
    assert torch.cuda.is_available()
    A._lib.load()
    groups, check = (NONE_GROUPS, False) if setting == "none" else (SETTINGS[setting][1], True)
    cases = {}
    with Recorder() as R:
        for fn, kw in groups:
            cases.update(fn(R, setting, check, **kw))
    return dict(setting=setting, env={} if setting == "none" else SETTINGS[setting][0], cases=cases)


if __name__ == "__main__":
    print("RESULT " + json.dumps(run(sys.argv[1])))
