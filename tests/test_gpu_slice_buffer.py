"""ops.SliceBuffer's shared gradient buffer (ops.ConcatSlicesFn, ConvFn's in-place `grad_dest` branch, ops.AddIntoFn), EXACTLY: a small
graph with D-DBPN's data flow (models/ddbpn.py: four parts, every growing prefix consumed, each consumer's output becoming the next
part) whose every stored value, forward and backward, is a small integer -- exact in bf16 and in fp16 -- so the gradient of every
leaf, part, weight and bias must EQUAL the float64 reference.  A gradient slice counted twice or dropped, which a whole-net comparison
in 16 bits cannot see (tests/ddbpn_ref.py), is off by an integer here.

Consumers, as in D-DBPN: prefix 1 by the no-bottleneck pattern of DenseProjection.nhwc (the `_srk_gacc` marker popped, then the prefix
used twice: by a transposed conv on the column path -- a 1x1 GEMM straight behind the prefix, the hazard models/ddbpn.py:58-61
documents -- and by a `sub`); prefixes 2 and 3 by a 1x1 ops.conv (a bottleneck: adds its data gradient in place); the full width by
ops.tail_conv.  "equal": the transposed conv has kernel 1 / stride 1, "strided": kernel 6 / stride 2 up and ops.conv_general back down."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N, H, W, COUNT = 2, 3, 5, 4
K, S, P = 6, 2, 2


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _ints(shape, gen, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).double()


def _sparse(shape, gen, share):
    """+-1 at about `share` of the positions, 0 elsewhere."""
    sign = torch.randint(0, 2, tuple(shape), generator=gen).double() * 2 - 1
    return sign * (torch.rand(tuple(shape), generator=gen, dtype=torch.float64) < share)


def _values(c, variant, seed=0):
    """Leaves (NCHW) and parameters (torch layouts) of the graph, float64 integers."""
    g = torch.Generator().manual_seed(seed)
    v = {nm: _ints((N, c, H, W), g, -2, 2) for nm in ("a", "b", "leaf1", "leaf2", "leaf3")}
    if variant == "equal":
        v["wu"], v["bu"] = _sparse((c, c, 1, 1), g, 3.0 / c), _ints((c,), g, -1, 1)
    else:
        v["wu"], v["bu"] = _sparse((c, c, K, K), g, 1.0 / (3 * c)), _ints((c,), g, -1, 1)      # [in][out][K][K]
        v["wd"], v["bd"] = _sparse((c, c, K, K), g, 1.0 / (12 * c)), _ints((c,), g, -1, 1)     # [out][in][K][K]
    for k in (2, 3):
        v[f"w{k}"], v[f"b{k}"] = _sparse((c, k * c, 1, 1), g, 2.0 / c), _ints((c,), g, -1, 1)
    v["wt"], v["bt"] = _sparse((3, COUNT * c, 3, 3), g, 1.0 / 27), _ints((3,), g, -1, 1)
    v["t"] = _ints((N, 3, H, W), g, -3, 3)                              # the loss: sum(image * t)
    return v


LEAVES = ("a", "b", "leaf1", "leaf2", "leaf3")


def _params(variant):
    return ("wu", "bu") + (("wd", "bd") if variant == "strided" else ()) + ("w2", "b2", "w3", "b3", "wt", "bt")


def _reference(v, variant):
    """float64 graph.  Returns (image, {name: gradient} for leaves, parts `p0..p3` and parameters, stored: every tensor the build keeps
    in 16 bits (activations, column tensors, their gradients), per: for each part {consumer's prefix length: that consumer's gradient of it})."""
    v = {k: t.clone().requires_grad_(k != "t") for k, t in v.items()}
    stored, contrib = [], {}

    def keep(t):
        stored.append(t.detach())
        t.register_hook(lambda g: stored.append(g.detach()))
        return t

    parts = []

    def cat(k):
        t = torch.cat(parts[:k], dim=1)
        t.register_hook(lambda g: contrib.__setitem__(k, g.detach()))
        return t

    parts.append(keep(v["a"] + v["b"]))
    x0 = cat(1)
    c = x0.shape[1]
    x = keep(x0.clone())                                                                # (the conv's own data gradient is stored too)
    if variant == "equal":
        cols = keep(F.conv2d(x, v["wu"].permute(1, 0, 2, 3)))                           # the GEMM's column tensor, K = 1
        b_0 = keep(cols + v["bu"].view(1, -1, 1, 1))
    else:
        cols = keep(torch.einsum("nihw,iokl->noklhw", x, v["wu"]).reshape(N, c * K * K, H * W))
        a_0 = keep(F.fold(cols, ((H - 1) * S - 2 * P + K, (W - 1) * S - 2 * P + K), K, stride=S, padding=P) + v["bu"].view(1, -1, 1, 1))
        ucols = F.unfold(a_0, K, stride=S, padding=P)
        ucols.register_hook(lambda g: stored.append(g.detach()))                       # the strided conv's data gradient before its fold
        b_0 = keep((v["wd"].reshape(c, -1) @ ucols).reshape(N, c, H, W) + v["bd"].view(1, -1, 1, 1))
    u = keep(b_0 - x0)
    parts.append(keep(u + v["leaf1"]))
    for k in (2, 3):
        u = keep(F.conv2d(cat(k), v[f"w{k}"], v[f"b{k}"]))
        parts.append(keep(u + v[f"leaf{k}"]))
    img = F.conv2d(cat(COUNT), v["wt"], v["bt"], padding=1)
    for p_ in parts:
        p_.retain_grad()
    (img * v["t"]).sum().backward()
    grads = {k: v[k].grad for k in LEAVES + _params(variant)}
    grads.update({f"p{i}": p_.grad for i, p_ in enumerate(parts)})
    per = [{k: g[:, i * c:(i + 1) * c] for k, g in contrib.items() if k > i} for i in range(COUNT)]     # part -> consumer -> its gradient
    return img.detach(), grads, stored, per


def _premise(v, variant):
    """Everything stored is an integer of at most 8 bits (exact in bf16, and so in fp16), partial sums of the gradient buffer included;
    every consumer reaches every part it covers with a gradient of comparable size."""
    img, grads, stored, per = _reference(v, variant)
    absum = [sum(g.abs() for g in d.values()) for d in per]                 # bounds every partial sum, whatever the order
    for t in stored + absum + [grads[k] for k in grads if k in LEAVES or k[0] == "p"]:
        assert torch.equal(t, t.to(torch.bfloat16).double()) and float(t.abs().max()) <= 256
    for i, d in enumerate(per):
        rms = [float(g.pow(2).mean().sqrt()) for g in d.values()]
        assert len(d) == COUNT - i and min(rms) > 0.25 and max(rms) <= 8 * min(rms), f"part {i}: consumers' gradients of RMS {rms}"
    for k in _params(variant):
        assert float(grads[k].abs().max()) < 2 ** 24 and float(grads[k].abs().max()) > 0, k
    return img, grads


def _nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


def _build(A, v, variant, dt, buf=None):
    """The graph on the build.  Returns (image, leaves, parameters, parts, buffer)."""
    ops = A.ops
    leaf = {k: _nhwc(v[k], dt).requires_grad_(True) for k in LEAVES}
    par = {k: v[k].float().cuda().requires_grad_(True) for k in _params(variant)}
    buf = ops.SliceBuffer(COUNT, accumulate_grads=True) if buf is None else buf
    parts = [ops.add_into(leaf["a"], leaf["b"], (buf, 0))]
    # prefix 1: DenseProjection.nhwc without a bottleneck
    x = ops.concat_slices(buf, parts[:1])
    x.__dict__.pop("_srk_gacc", None)
    if variant == "equal":
        b_0 = ops.conv_transpose_general(x, par["wu"], par["bu"], stride=1, pad=0)
    else:
        a_0 = ops.conv_transpose_general(x, par["wu"], par["bu"], stride=S, pad=P)
        b_0 = ops.conv_general(a_0, par["wd"], par["bd"], stride=S, pad=P)
    parts.append(ops.add_into(b_0.sub(x), leaf["leaf1"], (buf, 1)))
    for k in (2, 3):
        x = ops.concat_slices(buf, parts[:k])
        assert (x.__dict__.get("_srk_gacc") is not None) == buf.accumulate
        parts.append(ops.add_into(ops.conv(x, par[f"w{k}"], par[f"b{k}"]), leaf[f"leaf{k}"], (buf, k)))
    img = ops.tail_conv(ops.concat_slices(buf, parts), par["wt"], par["bt"])
    for p_ in parts:
        p_.retain_grad()
    return img, leaf, par, parts, buf


def _backward(A, v, img, leaf, par, parts):
    (img * v["t"].float().cuda()).sum().backward()
    A.ops.flush_wgrads()
    torch.cuda.synchronize()
    got = {k: t.grad.clone().permute(0, 3, 1, 2).double().cpu() for k, t in leaf.items()}
    got.update({f"p{i}": p_.grad.clone().permute(0, 3, 1, 2).double().cpu() for i, p_ in enumerate(parts)})
    got.update({k: t.grad.clone().double().cpu() for k, t in par.items()})
    return got


@pytest.mark.parametrize("gacc", [True, False], ids=["shared-buffer", "autograd-sums"])
@pytest.mark.parametrize("variant", ["equal", "strided"])
@pytest.mark.parametrize("c", [16, 32])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_gradients_equal_float64(A, monkeypatch, dt, c, variant, gacc):
    if not gacc:
        monkeypatch.setattr(A.ops, "_SLICE_GACC", False)
    v = _values(c, variant)
    img_ref, ref = _premise(v, variant)
    buf = None
    for rnd in range(2):                # the second pass: a fresh forward on the SAME buffer object, whose state the first backward reset
        img, leaf, par, parts, buf = _build(A, v, variant, dt, buf)
        assert buf.accumulate == gacc and buf.gbuf is None
        assert torch.equal(img.double().cpu(), img_ref)
        got = _backward(A, v, img, leaf, par, parts)
        assert buf.gbuf is None and buf.last_k is None
        assert set(got) == set(ref)
        for k in ref:
            assert got[k].shape == ref[k].shape, k
            assert torch.equal(got[k], ref[k]), f"pass {rnd}: gradient of {k}: {int((got[k] != ref[k]).sum())} of {ref[k].numel()} elements " \
                                                f"differ, max |diff| {float((got[k] - ref[k]).abs().max())}"


def test_out_of_order_consumer_raises(A):
    """Longest prefix first is what the shared buffer relies on: a consumer of a shorter prefix whose backward runs first must raise."""
    ops = A.ops
    v = _values(16, "equal")
    for in_place in (True, False):
        leaf = {k: _nhwc(v[k], torch.bfloat16).requires_grad_(True) for k in ("a", "b", "leaf1")}
        buf = ops.SliceBuffer(COUNT, accumulate_grads=True)
        parts = [ops.add_into(leaf["a"], leaf["b"], (buf, 0))]
        x1 = ops.concat_slices(buf, parts[:1])
        w1 = v["w2"][:, :16].float().cuda().requires_grad_(True)
        y1 = ops.conv(x1, w1, None) if in_place else x1 * 2
        parts.append(ops.add_into(y1, leaf["leaf1"], (buf, 1)))
        y2 = ops.conv(ops.concat_slices(buf, parts[:2]), v["w2"].float().cuda().requires_grad_(True), None)
        with pytest.raises(RuntimeError, match="SliceBuffer"):
            y1.float().sum().backward(retain_graph=True)        # prefix 1 before prefix 2
        del y2
