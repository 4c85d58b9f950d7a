"""Float64 statement of the VGG perceptual loss, written from its formulas and independent of sr_amd.vgg_loss:

  f(x) = slice((x - mean) / std),  mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225), the slice a run of 3x3 'same' convs, each
  followed by a ReLU, and 2x2 / stride 2 max-pools (floor) in torchvision's vgg16 / vgg19 `features` order;
  loss = rescale * mean((f(sr) - f(hr))^2)  or  rescale * mean(|f(sr) - f(hr)|).

Also the YARDSTICKS the GPU tests measure against (tests/test_gpu_vgg_loss.py): the same statement in float64 arithmetic with the weights,
the normalised input and every layer's output rounded to a 16-bit storage dtype (straight-through for the gradient), and the same
statement run in float32.  And the seeded weights and images of the tests, with one cache so that a reference is computed once."""
import functools
import math

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# layer -> the `features` modules in front of it, written out: C<n> a conv to n channels + ReLU, M a max-pool
SLICES = {
    ("vgg19", "relu1_2"): "C64 C64",
    ("vgg19", "relu2_2"): "C64 C64 M C128 C128",
    ("vgg19", "relu3_4"): "C64 C64 M C128 C128 M C256 C256 C256 C256",
    ("vgg19", "relu4_4"): "C64 C64 M C128 C128 M C256 C256 C256 C256 M C512 C512 C512 C512",
    ("vgg19", "relu5_4"): "C64 C64 M C128 C128 M C256 C256 C256 C256 M C512 C512 C512 C512 M C512 C512 C512 C512",
    ("vgg16", "relu1_2"): "C64 C64",
    ("vgg16", "relu2_2"): "C64 C64 M C128 C128",
    ("vgg16", "relu3_3"): "C64 C64 M C128 C128 M C256 C256 C256",
    ("vgg16", "relu4_3"): "C64 C64 M C128 C128 M C256 C256 C256 M C512 C512 C512",
}
NETS_LAYERS = tuple(SLICES)
CRITERIA = ("l2", "l1")
#: the smallest shapes at which each piece can still go wrong: relu5_4 ends at 1x1; odd sizes (floor pooling at every level) with
#: N = 1; an odd batch that ends at 2x1
SHAPES = ((2, 3, 16, 16), (1, 3, 37, 52), (3, 3, 33, 18))
RESCALE = 0.006


def steps(net, layer):
    """[(features index, Cin, Cout) | None (a pool)] of the slice."""
    out, i, cin = [], 0, 3
    for tok in SLICES[(net, layer)].split():
        if tok == "M":
            out.append(None)
            i += 1
        else:
            out.append((i, cin, int(tok[1:])))
            cin = int(tok[1:])
            i += 2
    return out


def make_weights(net, layer, seed=0):
    """The bare `features` state dict ({"<i>.weight", "<i>.bias"}) of the slice: He-normal weights (std sqrt(2 / (9 Cin))), biases uniform
    in +-0.1, seeded; fp32 (what a weights file holds)."""
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {}
    for s in steps(net, layer):
        if s is not None:
            i, cin, cout = s
            sd[f"{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
            sd[f"{i}.bias"] = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    return sd


def make_images(shape, seed=0):
    """hr uniform in [0, 1], sr = hr + 0.1 * normal noise (values outside [0, 1]: nothing is clamped); fp32."""
    g = torch.Generator().manual_seed(2000 + seed)
    hr = torch.rand(*shape, generator=g)
    sr = hr + 0.1 * torch.randn(*shape, generator=g)
    return sr, hr


def _rnd(x, storage):
    """x rounded to `storage` and back (None: untouched), straight-through for the gradient."""
    if storage is None:
        return x
    return x + (x.detach().to(storage).to(x.dtype) - x.detach())


def features(x, sd, net, layer, dtype=torch.float64, storage=None):
    """f(x) in `dtype` arithmetic; with `storage` the weights, the normalised input and every layer's output are rounded to it."""
    x = x.to(dtype)
    x = (x - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    x = _rnd(x, storage)
    for s in steps(net, layer):
        if s is None:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        else:
            w, b = sd[f"{s[0]}.weight"].to(dtype), sd[f"{s[0]}.bias"].to(dtype)
            x = _rnd(torch.clamp_min(F.conv2d(x, _rnd(w, storage), b, stride=1, padding=1), 0.0), storage)
    return x


def loss_of(fs, fh, criterion, rescale=RESCALE):
    d = fs - fh
    return rescale * ((d * d).sum() if criterion == "l2" else d.abs().sum()) / d.numel()


def loss(sr, hr, sd, net, layer, criterion="l2", rescale=RESCALE, dtype=torch.float64, storage=None):
    return loss_of(features(sr, sd, net, layer, dtype, storage), features(hr, sd, net, layer, dtype, storage), criterion, rescale)


def rel(a, b):
    """Relative L2 error of a against b (float64)."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def weights(net, layer):
    return make_weights(net, layer)


@functools.lru_cache(maxsize=None)
def images(shape):
    return make_images(shape)


def _evaluate(net, layer, shape, dtype, storage):
    sr, hr = images(shape)
    sd = weights(net, layer)
    s = sr.clone().to(dtype).requires_grad_(True)
    fs = features(s, sd, net, layer, dtype, storage)
    with torch.no_grad():
        fh = features(hr, sd, net, layer, dtype, storage)
    out = {"fs": fs.detach(), "fh": fh}
    for k, crit in enumerate(CRITERIA):
        v = loss_of(fs, fh, crit)
        g, = torch.autograd.grad(v, s, retain_graph=k + 1 < len(CRITERIA))
        out[crit] = (v.detach(), g)
    return out


@functools.lru_cache(maxsize=None)
def reference(net, layer, shape):
    """Float64: {"fs", "fh", "l2": (loss, d loss / d sr), "l1": (...)} for the test weights and images; computed once, never modified."""
    return _evaluate(net, layer, shape, torch.float64, None)


_STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16}


@functools.lru_cache(maxsize=None)
def yardstick(net, layer, shape, precision):
    """The errors against `reference` of a computation that is NOT the code under test and rounds like it: for "bf16" / "fp16" the float64
    statement with the weights, the normalised input and every layer's output rounded to that dtype; for "fp32" the statement run in
    float32.  {"features": rel L2, "l2": (loss rel error, gradient rel L2), "l1": (...)}."""
    ref = reference(net, layer, shape)
    y = _evaluate(net, layer, shape, torch.float32, None) if precision == "fp32" else \
        _evaluate(net, layer, shape, torch.float64, _STORAGE[precision])
    out = {"features": rel(y["fs"], ref["fs"])}
    for crit in CRITERIA:
        out[crit] = (abs(float(y[crit][0]) - float(ref[crit][0])) / abs(float(ref[crit][0])), rel(y[crit][1], ref[crit][1]))
    return out


def active_fraction(f):
    return float((f > 0).double().mean())
