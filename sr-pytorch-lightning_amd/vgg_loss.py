"""The VGG perceptual loss (SRGAN's / ESRGAN's feature-space loss; the reference's `VGGLoss`, losses/losses.py:54-117) on a FROZEN VGG-16 /
VGG-19 feature stack whose weights come from a file the user names.  Part of `ops` (re-exported there).  On the GPU the 3x3 conv + ReLU
layers are `srk_conv2d` launches on packs made once per (device, dtype) and the passes between them are csrc/vgg_loss.hip; plain torch
elsewhere.

  f(x)  = features_up_to_layer((x - mean) / std),  mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225)
  loss  = rescale * mean((f(sr) - f(hr))^2)   (criterion "l2", the reference's F.mse_loss)   or   rescale * mean(|f(sr) - f(hr)|)   ("l1")
NOTHING is clamped (like `l1` the loss takes sr as it comes), hr gets no gradient, and nothing here fetches weights from anywhere.

Layers are the reference's slices: vgg19 relu1_2, relu2_2, relu3_4, relu4_4, relu5_4; vgg16 relu1_2, relu2_2, relu3_3, relu4_3.  The images
must be at least 2^(pools before the layer) on each side.

HIP path (VGGLossFn): ONE prepare launch takes sr and hr to one NHWC batch of 2N normalised 16-channel images, so every weight is read
once per layer; conv + bias + ReLU per layer, a 2x2 max-pool kernel, per-workgroup double partials and one fixed-order finalize.  The
backward runs on the SR half only: data gradients with the ReLU mask of the saved SR activation, a gather-form max-pool backward (first
maximum, torch's rule), never a weight or bias gradient.  The chain carries the UN-normalised difference f(sr) - f(hr) (or its sign);
only the last kernel, in fp32, applies upstream * rescale * (2 | 1) / count, with `upstream` read on the device: folded in early the
factor underflows 16-bit storage.  No atomics, no host sync: bit-identical run to run and capturable once the packs exist (first call).
fp32 storage (the parity mode) runs each conv as one launch per `FP32_SLICE` reduction channels, for the accuracy of a blocked sum.
Memory: the SR half of every conv output before the layer's own, and the feature-loss gradient, stay alive between forward and backward
(INTEGRATION.md has the sizes); the HR half is dropped layer by layer."""
import math
import os

import torch
import torch.nn.functional as F

from . import _lib as L
from .ops import _DT, _f32c, _need_gpu, _stream, conv_raw, pack_conv, to_nchw      # (ops.py imports this module at its END: these exist by then)

__all__ = ["VGGFeatures", "VGGLoss", "VGGLossFn", "vgg_loss", "vgg_features", "vgg_loss_torch", "vgg_features_torch",
           "vgg_loss_parse_params", "vgg_pools", "max_pool_nhwc", "max_pool_nhwc_backward", "VGG_LOSS_PARAMS", "VGG_LAYERS", "VGG_MEAN", "VGG_STD"]

VGG_MEAN = (0.485, 0.456, 0.406)
VGG_STD = (0.229, 0.224, 0.225)
# torchvision's `features` configurations: output channels of a 3x3 conv (followed by a ReLU), "M" a 2x2 max-pool
_CFG = {"vgg16": (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512),
        "vgg19": (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512)}
#: net -> {layer: number of `features` modules the slice holds} (the reference's slices, losses/losses.py:133-140, 176-185)
VGG_LAYERS = {"vgg16": {"relu1_2": 4, "relu2_2": 9, "relu3_3": 16, "relu4_3": 23},
              "vgg19": {"relu1_2": 4, "relu2_2": 9, "relu3_4": 18, "relu4_4": 27, "relu5_4": 36}}
_CRITERIA = {"l2": L.SRK_VGG_L2, "l1": L.SRK_VGG_L1}
_PRECISIONS = {"32": torch.float32, "16": torch.float16, "bf16": torch.bfloat16}
#: parameter -> default (`vgg.weights` has none: it is required; `vgg.precision` defaults to the model's compute dtype)
VGG_LOSS_PARAMS = {"weights": None, "net": "vgg19", "layer": "relu2_2", "rescale": 0.006, "criterion": "l2", "precision": None}


def _conv_indices(net):
    """Index in torchvision's `features` of every conv of `net`, in order (vgg19: 0, 2, 5, 7, 10, ...)."""
    out, i = [], 0
    for c in _CFG[net]:
        if c == "M":
            i += 1
        else:
            out.append(i)
            i += 2
    return out


def _plan(net, layer):
    """The slice as a list of ("conv", features index, Cin, Cout) and ("pool",) steps; every conv is followed by its ReLU."""
    if net not in _CFG:
        raise ValueError(f"loss 'vgg': net={net!r} is not recognized (vgg19, vgg16)")
    if layer not in VGG_LAYERS[net]:
        raise ValueError(f"loss 'vgg': {net} has no layer {layer!r} (it has: {', '.join(VGG_LAYERS[net])})")
    end, steps, i, cin = VGG_LAYERS[net][layer], [], 0, 3
    for c in _CFG[net]:
        if i >= end:
            break
        if c == "M":
            steps.append(("pool",))
            i += 1
        else:
            steps.append(("conv", i, cin, c))
            cin = c
            i += 2
    assert i == end and steps[-1][0] == "conv"
    return steps


def vgg_pools(net, layer):
    """Number of max-pools before `layer` of `net`: the images must be at least 2^that on each side."""
    return sum(1 for s in _plan(net, layer) if s[0] == "pool")


def vgg_loss_parse_params(entries, default_precision=None):
    """`"vgg.<key>=<value>"` strings -> {"weights", "net", "layer", "rescale", "criterion", "dtype"}, defaults filled in
    (`default_precision`: the dtype a missing `vgg.precision` means; None: fp32).  Names, keys and the enumerated values are taken
    without regard to case or surrounding blanks; the path is taken as written.  ValueError for an entry of another form, a key `vgg`
    does not have, a net, criterion or precision that does not exist, a rescale that is not a finite float, a layer the net does not
    have, and a missing `vgg.weights`."""
    given = {}
    for entry in entries:
        left, sep, value = str(entry).strip().partition("=")
        name, dot, key = left.strip().partition(".")
        name, key, value = name.strip().lower(), key.strip().lower(), value.strip()
        if not sep or not dot or name != "vgg" or not key or not value:
            raise ValueError(f"loss parameter {entry!r} is not vgg.<key>=<value>")
        if key not in VGG_LOSS_PARAMS:
            raise ValueError(f"loss 'vgg' has no parameter {key} (it takes: {', '.join(VGG_LOSS_PARAMS)})")
        given[key] = value
    if "weights" not in given:
        raise ValueError("loss 'vgg' needs weights (e.g. loss_params=['vgg.weights=/data/vgg19.pth']): a torch.load-able state dict of "
                         "torchvision's vgg19 / vgg16; nothing is downloaded")
    net = given.get("net", VGG_LOSS_PARAMS["net"]).lower()
    layer = given.get("layer", VGG_LOSS_PARAMS["layer"]).lower()
    _plan(net, layer)
    criterion = given.get("criterion", VGG_LOSS_PARAMS["criterion"]).lower()
    if criterion not in _CRITERIA:
        raise ValueError(f"loss 'vgg': criterion={criterion!r} is not recognized (l2, l1)")
    try:
        rescale = float(given.get("rescale", VGG_LOSS_PARAMS["rescale"]))
    except (TypeError, ValueError):
        raise ValueError(f"loss 'vgg': rescale={given['rescale']!r} is not a float") from None
    if not math.isfinite(rescale):
        raise ValueError(f"loss 'vgg': rescale={rescale} is out of range (a finite float)")
    dtype = default_precision if default_precision is not None else torch.float32
    if "precision" in given:
        p = given["precision"].lower()
        if p not in _PRECISIONS:
            raise ValueError(f"loss 'vgg': precision={given['precision']!r} is not recognized (32, 16, bf16)")
        dtype = _PRECISIONS[p]
    return {"weights": given["weights"], "net": net, "layer": layer, "rescale": rescale, "criterion": criterion, "dtype": dtype}


class VGGFeatures:
    """The frozen conv weights of one slice (`net`, `layer`), and what each path makes of them once per (device, dtype).

    `weights`: a path to a torch.load-able state dict, or such a dict in memory: torchvision's `vgg19().state_dict()` /
    `vgg16().state_dict()` (keys `features.<i>.weight|bias`; `classifier.*` ignored) or the bare `features` state dict (keys
    `<i>.weight|bias`).  Only the convs of the slice are read and kept (fp32, on the CPU).  ValueError for a missing key, a wrong
    shape and a file of the other net.  Not an nn.Module: no optimizer, EMA, clipper or DDP wrapper ever sees these tensors."""

    def __init__(self, weights, net="vgg19", layer="relu2_2"):
        self.net, self.layer = str(net).lower(), str(layer).lower()
        self.plan = _plan(self.net, self.layer)
        self.pools = sum(1 for s in self.plan if s[0] == "pool")
        self.min_size = 2 ** self.pools
        self.channels = self.plan[-1][3]
        if isinstance(weights, (str, os.PathLike)):
            sd = torch.load(os.fspath(weights), map_location="cpu", weights_only=True)
        else:
            sd = weights
        if not isinstance(sd, dict):
            raise ValueError(f"loss 'vgg': the weights are a {type(sd).__name__}, not a state dict")
        self.convs = self._take(sd)
        self._packs, self._torch = {}, {}

    def _take(self, sd):
        prefix = "features." if any(str(k).startswith("features.") for k in sd) else ""
        other = "vgg16" if self.net == "vgg19" else "vgg19"
        mine, theirs = set(_conv_indices(self.net)), set(_conv_indices(other))
        has = lambda i: f"{prefix}{i}.weight" in sd                                    # noqa: E731
        if any(has(i) for i in theirs - mine) and not any(has(i) for i in mine - theirs):
            raise ValueError(f"loss 'vgg': the weights look like {other}'s (convs at features index "
                             f"{', '.join(str(i) for i in sorted(theirs - mine) if has(i))}), not {self.net}'s")
        convs = []
        for step in self.plan:
            if step[0] != "conv":
                continue
            _, i, cin, cout = step
            pair = []
            for kind, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
                key = f"{prefix}{i}.{kind}"
                if key not in sd:
                    raise ValueError(f"loss 'vgg': the weights have no {key!r} ({self.net} up to {self.layer} needs the convs at features "
                                     f"index {', '.join(str(s[1]) for s in self.plan if s[0] == 'conv')})")
                t = torch.as_tensor(sd[key])
                if tuple(t.shape) != shape:
                    raise ValueError(f"loss 'vgg': {key!r} has shape {tuple(t.shape)}, {self.net} needs {shape}")
                pair.append(t.detach().to(device="cpu", dtype=torch.float32).contiguous().clone())
            convs.append(tuple(pair))
        return convs

    def check_size(self, h, w):
        if h < self.min_size or w < self.min_size:
            raise ValueError(f"loss 'vgg': {self.net} {self.layer} has {self.pools} max-pools and needs images of at least "
                             f"{self.min_size} x {self.min_size}, got {h} x {w}")

    def weights(self, device, dtype):
        """[(w, b)] on `device` in `dtype` for the torch path (made once per pair)."""
        key = (str(device), dtype)
        ws = self._torch.get(key)
        if ws is None:
            ws = self._torch[key] = [(w.to(device=device, dtype=dtype), b.to(device=device, dtype=dtype)) for w, b in self.convs]
        return ws

    def packs(self, device, dtype):
        """[([forward packs], [data-gradient packs])] of the slice's convs on `device` in `dtype`, made by `srk_pack_conv_weights`
        launches on the FIRST call for that pair, none ever after (the weights never change; they join no PackGroup).  16-bit storage:
        one pack per direction.  fp32 storage: one pack per `FP32_SLICE` reduction channels (input channels forward, output channels
        for the data gradient; the first forward pack carries the bias): see `_conv_sliced`."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        key = (index, dtype)
        pk = self._packs.get(key)
        if pk is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the VGG weights are packed on the first eager call; call the loss once before capturing a graph")
            dev = torch.device("cuda", index)
            pk = []
            for w, b in self.convs:
                wd, bd = w.to(dev), b.to(dev)           # plain tensors, not parameters: no PackGroup takes them
                cout, cin = wd.shape[:2]
                s = FP32_SLICE if dtype == torch.float32 else max(cout, cin)
                pk.append(([pack_conv(wd[:, c:c + s].contiguous(), bd if c == 0 else None, dtype, cache=False) for c in range(0, cin, s)],
                           [pack_conv(wd[c:c + s].contiguous(), None, dtype, dgrad=True, cache=False) for c in range(0, cout, s)]))
            self._packs[key] = pk
        return pk

    def __getstate__(self):         # the packs hold device buffers: a copy of the object makes its own
        state = dict(self.__dict__)
        state["_packs"], state["_torch"] = {}, {}
        return state


def _check(sr, hr, features):
    if sr.dim() != 4 or sr.shape != hr.shape:
        raise ValueError(f"the VGG loss needs two N x 3 x H x W images of one shape, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    if sr.shape[1] != 3:
        raise ValueError(f"the VGG loss compares RGB images and needs 3 channels, got {sr.shape[1]}")
    if sr.shape[0] == 0:
        raise ValueError(f"the VGG loss needs non-empty images, got {tuple(sr.shape)}")
    features.check_size(sr.shape[-2], sr.shape[-1])


def _criterion(criterion):
    c = str(criterion).lower()
    if c not in _CRITERIA:
        raise ValueError(f"loss 'vgg': criterion={criterion!r} is not recognized (l2, l1)")
    return c


# --------------------------------------------------------------------------------------------
# torch path: the CPU path (fp32 or float64, differentiable in both images)
# --------------------------------------------------------------------------------------------
def vgg_features_torch(x, features):
    """f(x) in plain torch (N x C x h x w; float64 inputs stay float64, everything else computes in fp32; any device)."""
    dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    x = x.to(dt)
    mean = torch.tensor(VGG_MEAN, dtype=dt, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(VGG_STD, dtype=dt, device=x.device).view(1, 3, 1, 1)
    x = (x - mean) / std
    ws = iter(features.weights(x.device, dt))
    for step in features.plan:
        if step[0] == "pool":
            x = F.max_pool2d(x, 2, 2)
        else:
            w, b = next(ws)
            x = F.relu(F.conv2d(x, w, b, padding=1))
    return x


def vgg_loss_torch(sr, hr, features, rescale=0.006, criterion="l2"):
    """The VGG loss in plain torch (0-d; float64 inputs stay float64, everything else computes in fp32)."""
    c = _criterion(criterion)
    _check(sr, hr, features)
    d = vgg_features_torch(sr, features) - vgg_features_torch(hr, features)
    return float(rescale) * ((d * d).mean() if c == "l2" else d.abs().mean())


# --------------------------------------------------------------------------------------------
# HIP path (csrc/vgg_loss.hip around srk_conv2d)
# --------------------------------------------------------------------------------------------
def _prepare(sr, hr, dtype):
    """sr (and hr, unless None) NCHW fp32 -> [2N | N][H][W][16] normalised, in ONE launch."""
    n, _, h, w = sr.shape
    x = torch.empty(((1 if hr is None else 2) * n, h, w, 16), dtype=dtype, device=sr.device)
    a = L.VggPrepareArgs(sr=sr.data_ptr(), hr=0 if hr is None else hr.data_ptr(), dst=x.data_ptr(), N=n, H=h, W=w, dtype=_DT[dtype])
    L.call("srk_vgg_prepare", a, _stream())
    return x


def _pool(x, y=None, gy=None, gx=None, relu_mask=False):
    n, h, w, c = x.shape
    a = L.VggPoolArgs(x=x.data_ptr(), y=0 if y is None else y.data_ptr(), gy=0 if gy is None else gy.data_ptr(),
                      gx=0 if gx is None else gx.data_ptr(), N=n, H=h, W=w, C=c, relu_mask=int(relu_mask), dtype=_DT[x.dtype])
    L.call("srk_vgg_pool_bwd" if y is None else "srk_vgg_pool_fwd", a, _stream())


def max_pool_nhwc(x):
    """nn.MaxPool2d(2, 2) of a dense NHWC tensor (channels a multiple of 16; bf16 / fp16 / fp32)."""
    _need_gpu(x)
    n, h, w, c = x.shape
    y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    _pool(x, y=y)
    return y


def max_pool_nhwc_backward(x, gy, relu_mask=False):
    """The gradient of `max_pool_nhwc(x)` with respect to x given the one of its output (first maximum of a window takes it); with
    `relu_mask` also zero where x <= 0."""
    _need_gpu(x)
    gx = torch.empty_like(x)
    _pool(x, gy=gy, gx=gx, relu_mask=relu_mask)
    return gx


#: fp32 storage only: reduction channels per srk_conv2d launch of a conv of the stack.  srk_conv2d adds the 9 x Cin products of an
#: output in ONE sequential fp32 chain (4,608 terms at 512 channels), whose rounding error grows with its length; fp32 is the parity
#: mode, so there the chain is cut into launches over channel slices that add up through `res`: a blocked sum, like torch's own.
#: 16 (chains of 144) is the narrowest slice srk_conv2d takes and brings the error against float64 down to that of torch's fp32 CPU
#: convolution; wider slices are faster and less accurate (profiles/vgg_loss.txt).
FP32_SLICE = 16


def _conv_sliced(x, pks, out, *, relu=False, mask=None):
    """out = conv(x) through the packs `pks` (+ the first one's bias and a ReLU when `relu`; `mask`: the ReLU-backward mask).  One
    pack: one launch with everything in its epilogue.  Several (fp32 storage): pack i takes the i-th slice of x's channels, launches
    after the first add to `out` in place, the mask rides on the last one, and the ReLU, which the epilogue applies BEFORE `res`,
    follows as an in-place pass."""
    b, h, w, c = x.shape
    cout = out.shape[3]
    if len(pks) == 1:
        conv_raw(x, pks[0], N=b, H=h, W=w, Cin=c, Cout=cout, out=out, relu=relu, use_bias=relu, mask=mask)
        return
    s = c // len(pks)
    for i, pk in enumerate(pks):
        conv_raw(x[..., i * s:(i + 1) * s], pk, N=b, H=h, W=w, Cin=s, Cout=cout, out=out, use_bias=relu and i == 0,
                 res=out if i else None, mask=mask if i == len(pks) - 1 else None)
    if relu:
        L.call("srk_vgg_relu", L.VggReluArgs(x=out.data_ptr(), n=out.numel(), dtype=_DT[out.dtype]), _stream())


def _stack(features, x, keep):
    """The slice on the NHWC batch `x`.  keep > 0: also the first `keep` images of every conv's output (post-ReLU) but the last, each
    in a tensor of its own, so that the rest of the batch is freed as the stack moves on."""
    packs = features.packs(x.device, x.dtype)
    saved, ci = [], 0
    for step in features.plan:
        b, h, w, c = x.shape
        if step[0] == "pool":
            x = max_pool_nhwc(x)
            continue
        cout = step[3]
        y = torch.empty((b, h, w, cout), dtype=x.dtype, device=x.device)
        _conv_sliced(x, packs[ci][0], y, relu=True)
        ci += 1
        if keep and ci < len(packs):
            saved.append(y[:keep].clone() if keep < b else y)
        x = y
    return x, saved


def _feat_args(fs, fh, criterion, **kw):
    return L.VggFeatArgs(fs=fs.data_ptr(), fh=fh.data_ptr(), n=fs.numel(), criterion=_CRITERIA[criterion], dtype=_DT[fs.dtype], **kw)


class VGGLossFn(torch.autograd.Function):
    """apply(sr, hr, features, rescale, criterion, dtype): the VGG loss on the HIP path (module docstring).  Kept for the backward: the
    un-normalised feature-loss gradient and the SR half of every conv output but the last, in `dtype`."""

    @staticmethod
    def forward(ctx, sr, hr, features, rescale, criterion, dtype):
        _need_gpu(sr)
        _need_gpu(hr)
        _check(sr, hr, features)
        n = sr.shape[0]
        need = bool(ctx.needs_input_grad[0])
        f, saved = _stack(features, _prepare(_f32c(sr), _f32c(hr), dtype), n if need else 0)
        fs, fh = f[:n], f[n:]
        blocks = L.load().srk_vgg_blocks(fs.numel() * fs.element_size() // 16)
        partial = torch.empty(blocks, dtype=torch.float64, device=sr.device)
        loss = torch.empty((), dtype=torch.float32, device=sr.device)
        a = _feat_args(fs, fh, criterion, partial=partial.data_ptr(), loss=loss.data_ptr(), rescale=float(rescale))
        L.call("srk_vgg_feat_fwd", a, _stream())
        L.call("srk_vgg_feat_finalize", a, _stream())
        if need:
            gf = torch.empty(fs.shape, dtype=dtype, device=sr.device)
            L.call("srk_vgg_feat_grad", _feat_args(fs, fh, criterion, gf=gf.data_ptr()), _stream())
            ctx.save_for_backward(gf, *saved)
            ctx.features = features
            ctx.scale = float(rescale) * (2.0 if criterion == "l2" else 1.0) / fs.numel()
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        g, *acts = ctx.saved_tensors
        features = ctx.features
        packs = features.packs(g.device, g.dtype)
        gout = gout.detach().float().contiguous()
        plan = features.plan
        convs = [k for k, s in enumerate(plan) if s[0] == "conv"]
        # g is the gradient with respect to the PRE-activation of the conv (or the output of the pool) it stands behind
        for k in range(len(plan) - 1, -1, -1):
            ci = convs.index(k) if plan[k][0] == "conv" else None
            if ci is None:                              # pool k reads conv k - 1's activation: through the pool and that ReLU in one pass
                g = max_pool_nhwc_backward(acts[convs.index(k - 1)], g, relu_mask=True)
                continue
            n, h, w, cout = g.shape
            cin = max(16, plan[k][2])
            mask = acts[ci - 1] if (k > 0 and plan[k - 1][0] == "conv") else None      # the ReLU of the conv that feeds this one
            gx = torch.empty((n, h, w, cin), dtype=g.dtype, device=g.device)
            _conv_sliced(g, packs[ci][1], gx, mask=mask)
            g = gx
        n, h, w, _ = g.shape
        grad = torch.empty((n, 3, h, w), dtype=torch.float32, device=g.device)
        a = L.VggImageGradArgs(g=g.data_ptr(), gout=gout.data_ptr(), grad=grad.data_ptr(), scale=ctx.scale, N=n, H=h, W=w, dtype=_DT[g.dtype])
        L.call("srk_vgg_image_grad", a, _stream())
        return grad, None, None, None, None, None


def _hip_ok(sr, hr):
    return sr.is_cuda and hr.is_cuda and not hr.requires_grad and sr.dtype in (torch.float32, torch.float16, torch.bfloat16)


def vgg_loss(sr, hr, features, rescale=0.006, criterion="l2", dtype=torch.float32):
    """The VGG loss of sr against hr on the slice `features` holds: HIP for CUDA tensors (feature stack stored in `dtype`: fp32, fp16 or
    bf16), `vgg_loss_torch` for CPU tensors, float64 and a target that needs a gradient."""
    c = _criterion(criterion)
    _check(sr, hr, features)
    if _hip_ok(sr, hr):
        if dtype not in _DT:
            raise ValueError(f"loss 'vgg': storage dtype {dtype} is not one of fp32, fp16, bf16")
        return VGGLossFn.apply(sr, hr, features, float(rescale), c, dtype)
    return vgg_loss_torch(sr, hr, features, rescale, c)


def vgg_features(x, features, dtype=torch.float32):
    """f(x), no gradient, as N x C x h x w fp32: through the HIP stack in `dtype` for a CUDA tensor, `vgg_features_torch` otherwise."""
    with torch.no_grad():
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] == 0:
            raise ValueError(f"the VGG features need N x 3 x H x W images, got {tuple(x.shape)}")
        features.check_size(x.shape[-2], x.shape[-1])
        if not x.is_cuda or x.dtype == torch.float64:
            return vgg_features_torch(x, features)
        f, _ = _stack(features, _prepare(_f32c(x), None, dtype), 0)
        return to_nchw(f)


class VGGLoss:
    """The `vgg` term of a loss string as a callable: owns its `VGGFeatures` (loaded here, moved / packed on the first call, on the
    device of that call's tensors).  Deliberately NOT an nn.Module: the model's state_dict, parameters and checkpoints do not change."""

    def __init__(self, weights, net="vgg19", layer="relu2_2", rescale=0.006, criterion="l2", dtype=torch.float32):
        self.features = VGGFeatures(weights, net, layer)
        self.rescale, self.criterion, self.dtype = float(rescale), _criterion(criterion), dtype
        self.__name__ = "_vgg_loss"

    def __call__(self, sr, hr):
        return vgg_loss(sr, hr, self.features, self.rescale, self.criterion, self.dtype)
