"""Shared helper of the D-DBPN whole-step tests (test_ddbpn_ref_cpu.py, test_gpu_ddbpn_step.py) -- TEST INFRASTRUCTURE, never
imported by the product.

The reference is the float64 oracle on `DDBPN(scale_factor=s)` at its default initialisation under `torch.manual_seed(0)`: D-DBPN's
loop (oracle/functional.py `ddbpn_forward`) restated from its public pieces so that the 11 parts of the two concatenations (6 HR,
5 LR feature maps) are at hand and their gradients can be read.  Input and target are `torch.rand` from a generator seeded 1234
(LR first, then HR), the loss is L1.  `run` has four uses:

* clean          float64 arithmetic: the reference (`run(s)`); test_ddbpn_ref_cpu.py asserts it IS `OF.ddbpn_forward`, bit for bit;
* fp32           the same loop in fp32 arithmetic on the CPU (`arith=torch.float32`): what fp32 sums cost;
* storage noise  float64 arithmetic with every tensor the build STORES in 16 bits rounded there, in both directions (`store=dt`):
                 the 4-D weights as packed (their gradients stay fp32), the head's input, the output of every conv / PReLU / sub /
                 add, and every activation gradient; biases and slopes stay fp32; the loss is scaled by `LOSS_SCALE` (1024) as the
                 fp16 tests of the project do.  `round_cols` also rounds the column tensor between the GEMM and the fold of the
                 transposed convs (and of the strided convs' data gradient), which exists at scales 2 and 8 only (scale 4 in 16 bits
                 runs on the direct kernels, csrc/proj.hip);
* planted errors switches of the loop for the CPU test alone:
    "slice"   one concatenation consumer's gradient of one slice counted twice (`SLICE_PLANTS`: a bottleneck consumer of each buffer)
              -- what an in-place add into the shared gradient buffer that autograd sums AGAIN would do (models/ddbpn.py:58-61);
    "double"  the hazard of models/ddbpn.py:58-61 itself, in the two no-bottleneck units (upmodules.1, downmodules.0): the unit input's
              conv_1 consumer adds its data gradient into the shared buffer AND autograd sums the returned buffer again with the
              `sub` branch's gradient, so part 0 of either buffer receives 2 (S + g_conv_1) + g_sub for S + g_conv_1 + g_sub (S: the
              other consumers' sum);
    "nosub"   the `b_0.sub(x)` branch dropped in those two units.

Limits (test_ddbpn_ref_cpu.py asserts the conditions, the GPU test recomputes every number from here):

  LIMIT32 = 16 x the fp32 baseline (worst relative L2 of the fp32 run against float64 over parameter and part gradients; tensors
            under 256 elements on the scale of the largest gradient, like `grad_err` of test_gpu_models.py).  16: MFMA and fold
            summation orders other than the CPU's, and a rare PReLU / L1 sign flip.  Conditions: <= 1e-3, and at most a quarter of
            the smallest movement a "slice" error causes on the gradient of the part it touches.
  LIMIT16 = eval_ref.MARGIN (2.0) x the 16-bit baseline (worst relative L2 over parameter tensors of >= 256 elements, both noise
            variants), per scale and dtype.  Condition: under "double" and under "nosub" at least five parameter tensors move by more
            than 2 x LIMIT16.

Measured on the CPU (`python tests/ddbpn_ref.py` prints this table):

  scale  fp32 baseline   LIMIT32   slice: part movement (parameters)      double: 5th largest   nosub: 5th largest
  -----  -------------  --------  -------------------------------------  -------------------  ------------------
  x2          5.36e-07   8.6e-06  0.0139 (0.0201)  0.2188 (0.2429)                     1.038               0.450
  x4          8.57e-07   1.4e-05  0.0072 (0.0078)  0.1980 (0.2412)                     1.005               0.428
  x8          1.29e-06   2.1e-05  0.0036 (0.0052)  0.2236 (0.2506)                     0.985               0.406

  scale  dtype  16-bit baseline: worst (median) per noise variant   LIMIT16   tensors > 2 x LIMIT16: double  nosub
  -----  -----  ---------------------------------------------------  -------  -----------------------------------
  x2     fp16   0.0331 (0.0048)  0.0331 (0.0029)                      0.0662                              8     22
  x2     bf16   0.0561 (0.0192)  0.0577 (0.0225)                      0.1155                              8      7
  x4     fp16   0.0284 (0.0030)                                       0.0568                              8     13
  x4     bf16   0.0324 (0.0143)                                       0.0649                              8     10
  x8     fp16   0.0104 (0.0063)  0.0131 (0.0047)                      0.0262                              8     29
  x8     bf16   0.0846 (0.0185)  0.0412 (0.0182)                      0.1692                              8      5
"""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))       # (run as a script: the repository root)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import functional as OF  # noqa: E402
import eval_ref as ER  # noqa: E402

SCALES = (2, 4, 8)
LR_SHAPE = {2: (2, 9, 11), 4: (2, 6, 7), 8: (2, 4, 5)}          # (N, h, w) of the LR batch
INPUT_SEED = 1234
LOSS_SCALE = 1024.0
DEPTH = 6
SMALL = 256                       # parameter tensors below this many elements: judged on the scale of the largest gradient / not at all
MARGIN32 = 16.0
DTYPES16 = (torch.float16, torch.bfloat16)
NO_BOTTLENECK = ("upmodules.1", "downmodules.0")
# (consumer unit, slice index) of the "slice" error: a bottleneck consumer of the HR buffer's prefix 3 and one of the LR buffer's prefix 3
SLICE_PLANTS = (("downmodules.2", 1), ("upmodules.3", 0))
PART_NAMES = tuple(f"h{i}" for i in range(DEPTH)) + tuple(f"l{i}" for i in range(DEPTH - 1))


@functools.lru_cache(maxsize=None)
def inputs(scale):
    """(state dict, LR batch, HR target) of a case: fp32 tensors, the model's default initialisation under seed 0."""
    import sr_amd
    torch.manual_seed(0)
    m = sr_amd.DDBPN(scale_factor=scale)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    trainable = tuple(k for k, p in m.named_parameters() if p.requires_grad)
    n, h, w = LR_SHAPE[scale]
    g = torch.Generator().manual_seed(INPUT_SEED)
    x = torch.rand(n, 3, h, w, generator=g)
    hr = torch.rand(n, 3, h * scale, w * scale, generator=g)
    return sd, trainable, x, hr


class _Q(torch.autograd.Function):
    """Storage rounding: the value (unless `grad_only`) and its gradient pass through `dt`."""

    @staticmethod
    def forward(ctx, t, dt, grad_only):
        ctx.dt = dt
        return t.view_as(t) if grad_only else t.to(dt).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).to(g.dtype), None, None


class _GradScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, f):
        ctx.f = f
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.f, None


class _Hooks:
    """What one run does beyond the clean loop."""

    def __init__(self, store=None, round_cols=False, plant=None, scale=4):
        self.store, self.plant = store, plant
        self.cols = store is not None and round_cols and scale != 4
        self.plain = store is None and plant is None

    def q(self, t, grad_only=False):
        return t if self.store is None else _Q.apply(t, self.store, grad_only)

    def w(self, w):
        """A 4-D weight as the build packs it: rounded, its gradient (fp32 in the build) untouched."""
        if self.store is None:
            return w
        return w + (w.detach().to(self.store).to(w.dtype) - w.detach())


def _proj_conv(sd, prefix, x, scale, up, hk):
    """The projection conv `prefix` (no PReLU); with `hk.cols` in the build's two stages, the column tensor stored in between."""
    k, s, p = OF.DDBPN_PROJ[scale]
    w, b = hk.w(sd[prefix + ".weight"]), sd[prefix + ".bias"]
    if not hk.cols:
        return F.conv_transpose2d(x, w, b, stride=s, padding=p) if up else F.conv2d(x, w, b, stride=s, padding=p)
    n, _, h, wd = x.shape
    if up:
        co = w.shape[1]
        cols = torch.einsum("nihw,iokl->noklhw", x, w).reshape(n, co * k * k, h * wd)
        ho, wo = (h - 1) * s - 2 * p + k, (wd - 1) * s - 2 * p + k
        return F.fold(hk.q(cols), (ho, wo), k, stride=s, padding=p) + b.view(1, -1, 1, 1)
    co = w.shape[0]
    ho, wo = (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1
    cols = hk.q(F.unfold(x, k, stride=s, padding=p), grad_only=True)      # a copy forward; its gradient is the GEMM's stored output
    return (w.reshape(co, -1) @ cols).reshape(n, co, ho, wo) + b.view(1, -1, 1, 1)


def _unit(sd, prefix, x, scale, up, bottleneck, hk):
    """`OF.dense_projection` with the hooks between its steps."""
    def proj(name, t, up_):
        return hk.q(OF.prelu(sd, f"{prefix}.{name}.1", hk.q(_proj_conv(sd, f"{prefix}.{name}.0", t, scale, up_, hk))))
    if bottleneck:
        y = F.conv2d(x, hk.w(sd[prefix + ".bottleneck.0.weight"]), sd[prefix + ".bottleneck.0.bias"])
        x = hk.q(OF.prelu(sd, prefix + ".bottleneck.1", hk.q(y)))
    planted = prefix in NO_BOTTLENECK
    a_0 = proj("conv_1", x, up)
    b_0 = proj("conv_2", a_0, not up)
    # "double": the part's gradient is doubled where it is made (run), all but this branch's share of it
    x_sub = _GradScale.apply(x, 0.5) if (planted and hk.plant == "double") else x
    e = b_0 if (planted and hk.plant == "nosub") else hk.q(b_0.sub(x_sub))
    a_1 = proj("conv_3", e, up)
    return hk.q(a_0.add(a_1))


def _rel(got, ref, gmax=None):
    """Relative L2; a tensor under SMALL elements on the scale of the largest gradient (grad_err of test_gpu_models.py)."""
    got, ref = got.double().flatten(), ref.double().flatten()
    den = float(ref.norm())
    if gmax is not None and ref.numel() < SMALL:
        den = max(den, 0.05 * gmax * ref.numel() ** 0.5)
    return float((got - ref).norm()) / (den + 1e-300)


def run(scale, *, arith=torch.float64, store=None, round_cols=False, plant=None, slice_plant=None):
    """One training step of the reference loop.  Returns dict(image, loss, grads {parameter name: gradient}, parts {PART_NAMES:
    gradient}), all in `arith`, gradients of the UNscaled loss."""
    sd0, trainable, x, hr = inputs(scale)
    sd = {k: (v.to(arith, copy=True) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    for k in trainable:
        sd[k].requires_grad_(True)
    hk = _Hooks(store, round_cols, plant, scale)
    loss_scale = LOSS_SCALE if store is not None else 1.0

    def unit(prefix, t, up, bottleneck):
        if hk.plain:
            return OF.dense_projection(sd, prefix, t, scale, up, bottleneck)
        return _unit(sd, prefix, t, scale, up, bottleneck, hk)

    def cat(parts, consumer):
        if plant == "slice" and consumer == slice_plant[0]:
            parts = [_GradScale.apply(p_, 2.0) if i == slice_plant[1] else p_ for i, p_ in enumerate(parts)]
        return torch.cat(parts, dim=1)

    t = hk.q(OF.mean_shift(sd, "sub_mean", x.to(arith)))
    t = hk.q(OF.prelu(sd, "initial.1", hk.q(F.conv2d(t, hk.w(sd["initial.0.weight"]), sd["initial.0.bias"], padding=1))))
    t = hk.q(OF.prelu(sd, "initial.3", hk.q(F.conv2d(t, hk.w(sd["initial.2.weight"]), sd["initial.2.bias"]))))
    h_list, l_list, made = [], [], []

    def part(lst, p_):
        made.append(p_)
        p_.retain_grad()
        # "double": part 0 of either buffer is the input of a no-bottleneck unit (NO_BOTTLENECK), see the module docstring
        lst.append(_GradScale.apply(p_, 2.0) if (plant == "double" and not lst) else p_)

    for i in range(DEPTH - 1):
        l = t if i == 0 else cat(l_list, f"upmodules.{i}")
        part(h_list, unit(f"upmodules.{i}", l, True, i > 1))
        part(l_list, unit(f"downmodules.{i}", cat(h_list, f"downmodules.{i}"), False, i != 0))
    part(h_list, unit(f"upmodules.{DEPTH - 1}", cat(l_list, f"upmodules.{DEPTH - 1}"), True, True))
    rec = F.conv2d(cat(h_list, "reconstruction.0"), hk.w(sd["reconstruction.0.weight"]), sd["reconstruction.0.bias"], padding=1)
    y = hk.q(OF.mean_shift(sd, "add_mean", rec), grad_only=True)         # the image is fp32; its gradient enters the tail conv in 16 bits
    loss = F.l1_loss(y, hr.to(arith))
    (loss * loss_scale).backward()
    return dict(image=y.detach(), loss=float(loss.detach()),
                grads={k: sd[k].grad / loss_scale for k in trainable},
                parts={nm: p_.grad / loss_scale for nm, p_ in zip(PART_NAMES, made[0::2] + made[1::2])})


@functools.lru_cache(maxsize=None)
def reference(scale):
    """The clean float64 run, computed once and shared (read-only) by every test that needs it."""
    return run(scale)


def gmax_of(ref):
    return max(float(g.abs().max()) for g in ref["grads"].values())


def errors(got, ref, *, parts=True, small=True):
    """{name: relative L2} of `got`'s parameter (and part) gradients against `ref`'s; `small` False leaves out tensors under SMALL elements."""
    gmax = gmax_of(ref)
    out = {}
    for k, g in ref["grads"].items():
        if small or g.numel() >= SMALL:
            out[k] = _rel(got["grads"][k], g, gmax)
    if parts:
        for k, g in ref["parts"].items():
            out["part:" + k] = _rel(got["parts"][k], g)
    return out


@functools.lru_cache(maxsize=None)
def baseline32(scale):
    return max(errors(run(scale, arith=torch.float32), reference(scale)).values())


def limit32(scale):
    return MARGIN32 * baseline32(scale)


@functools.lru_cache(maxsize=None)
def baselines16(scale, dt):
    """(worst, median) relative L2 over the sizeable parameter tensors per noise variant: [(without, with) the column tensor rounded]."""
    out = []
    for cols in ((False,) if scale == 4 else (False, True)):                 # scale 4 has no column tensor in 16 bits
        e = sorted(errors(run(scale, store=dt, round_cols=cols), reference(scale), parts=False, small=False).values())
        out.append((e[-1], e[len(e) // 2]))
    return tuple(out)


def limit16(scale, dt):
    return ER.MARGIN * max(w for w, _ in baselines16(scale, dt))


@functools.lru_cache(maxsize=None)
def slice_movement(scale):
    """Per SLICE_PLANTS entry: (relative L2 movement of the touched part's gradient, worst movement of a parameter gradient)."""
    ref = reference(scale)
    out = []
    for unit, idx in SLICE_PLANTS:
        got = run(scale, plant="slice", slice_plant=(unit, idx))
        part = ("l" if unit.startswith("up") else "h") + str(idx)
        out.append((_rel(got["parts"][part], ref["parts"][part]), max(errors(got, ref, parts=False).values())))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gross_signature(scale, plant):
    """Relative L2 movements of the sizeable parameter gradients under a gross planted error, largest first."""
    return tuple(sorted(errors(run(scale, plant=plant), reference(scale), parts=False, small=False).values(), reverse=True))


def table():
    name = {torch.float16: "fp16", torch.bfloat16: "bf16"}
    lines = ["  scale  fp32 baseline   LIMIT32   slice: part movement (parameters)      double: 5th largest   nosub: 5th largest",
             "  -----  -------------  --------  -------------------------------------  -------------------  ------------------"]
    for s in SCALES:
        mv = "  ".join(f"{p:.4f} ({q:.4f})" for p, q in slice_movement(s))
        lines.append(f"  x{s}     {baseline32(s):13.2e}  {limit32(s):8.1e}  {mv:37s}  {gross_signature(s, 'double')[4]:19.3f}  "
                     f"{gross_signature(s, 'nosub')[4]:18.3f}")
    lines += ["", "  scale  dtype  16-bit baseline: worst (median) per noise variant   LIMIT16   tensors > 2 x LIMIT16: double  nosub",
              "  -----  -----  ---------------------------------------------------  -------  -----------------------------------"]
    for s in SCALES:
        for dt in DTYPES16:
            b = "  ".join(f"{w:.4f} ({m:.4f})" for w, m in baselines16(s, dt))
            lim = limit16(s, dt)
            cnt = [sum(e > 2 * lim for e in gross_signature(s, pl)) for pl in ("double", "nosub")]
            lines.append(f"  x{s}     {name[dt]}   {b:51s}  {lim:7.4f}  {cnt[0]:29d}  {cnt[1]:5d}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(table())
