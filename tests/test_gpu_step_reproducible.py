"""A training step repeats itself bit for bit: every launch of forward, loss, backward and optimizer sums in a fixed order, in fp32, bf16
and fp16, and a replayed graph gives the bits of the launch-by-launch loop ("Reproducibility").

Everything here is compared by BITS: torch.equal on the integer view of the tensors, so that NaN and -0 are compared too; no tolerance,
no element left out.  Only run 1 of the raw weight gradient is also held against float64, so that "reproducible" cannot mean
"reproducibly wrong".

a. `grads.wgrad_raw` launched four times on the same operands (fp32 takes the generic kernel, 32 workgroups whose four K-group waves
   meet in every address; 16-bit the slab kernels), and once more in a child process under SRK_NO_WS=1, where the 16-bit shapes take the
   generic kernel too (the knob is read once per process: tests/test_gpu_dispatch_sides.py starts its children the same way);
b. forward + L1 + backward of every model class, four times from one set of weights: the first parameter whose gradient differs is
   named, which is what locates a kernel that is not reproducible;
c. `Trainer.fit`, six Adam steps: eager twice from the same seed, and replayed from a captured graph.

python tests/test_gpu_step_reproducible.py wgrad-child     -> one line "RESULT {json}" (the child of a.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dispatch_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = D.ROOT
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))

RUNS = 4
WGRAD_N = 8               # images of 24 x 24: 32 pixel tiles of 16 x 16
WGRAD_SHAPES = [(3, 64, 64), (3, 16, 48), (3, 32, 32), (1, 64, 32), (1, 128, 96)]           # (k, Cin, Cout)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CHILD_TIMEOUT = 120


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


def _bits(t):
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _float_bits(values):
    return np.asarray(values, dtype=np.float32).view(np.int32).tolist()


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. the raw weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------------
_WGRAD_REF = {}           # (dtype name, shape) -> (operands on the CPU, float64 dw, float64 db): computed once, never modified


def _wgrad_operands(dtname, k, cin, cout):
    key = (dtname, k, cin, cout)
    if key not in _WGRAD_REF:
        dt = DTYPES[dtname]
        g = torch.Generator().manual_seed(D._seed("repro-wgrad", k, cin, cout))
        x = (torch.rand(WGRAD_N, 24, 24, cin, generator=g) - 0.5).to(dt)
        dy = (torch.rand(WGRAD_N, 24, 24, cout, generator=g) - 0.5).to(dt)
        ref_w = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (cout, cin, k, k), dy.double().permute(0, 3, 1, 2), padding=k // 2)
        ref_b = dy.double().sum((0, 1, 2))
        _WGRAD_REF[key] = (x, dy, ref_w, ref_b)
    return _WGRAD_REF[key]


def _wgrad_runs(A, dtname, k, cin, cout, recorder=None):
    """RUNS launches on the same operands -> [(dw, db)] on the device (outputs prefilled with NaN), and the kernel names."""
    x, dy, _, _ = _wgrad_operands(dtname, k, cin, cout)
    x, dy = x.cuda(), dy.cuda()
    runs, names = [], []
    for _ in range(RUNS):
        dw = torch.full((cout, cin, k, k), float("nan"), device="cuda")
        db = torch.full((cout,), float("nan"), device="cuda")
        if recorder is not None:
            recorder.take()
        A.ops.wgrad_raw(x, dy, N=WGRAD_N, H=24, W=24, Cin=cin, Cout=cout, k=k, w_shape=(cout, cin, k, k), out_w=dw, out_b=db)
        torch.cuda.synchronize()
        if recorder is not None:
            names.append(D._names(recorder.take(), "srk_conv2d_wgrad")[-1])
        runs.append((dw, db))
    return runs, names


def _wgrad_verdict(dtname, k, cin, cout, runs):
    """(runs that differ from run 1 in dw, in db, worst error of run 1 / its bound)."""
    _, _, ref_w, ref_b = _wgrad_operands(dtname, k, cin, cout)
    dw1, db1 = runs[0]
    bad_w = [i + 1 for i, (dw, _) in enumerate(runs) if not same_bits(dw, dw1)]
    bad_b = [i + 1 for i, (_, db) in enumerate(runs) if not same_bits(db, db1)]
    # the bound of test_gpu_wgrad_group.py::test_grouped_matches_per_layer_and_float64: fp32 accumulation of <= 4,608 products per entry
    ew = float((dw1.double().cpu() - ref_w).abs().max()) / (1e-4 * float(ref_w.abs().max()))
    eb = float((db1.double().cpu() - ref_b).abs().max()) / (1e-4 * float(ref_b.abs().max()))
    finite = bool(torch.isfinite(dw1).all() and torch.isfinite(db1).all())
    return bad_w, bad_b, (max(ew, eb) if finite else float("inf"))


@pytest.mark.parametrize("k,cin,cout", WGRAD_SHAPES, ids=[f"{k}x{k}-{ci}to{co}" for k, ci, co in WGRAD_SHAPES])
@pytest.mark.parametrize("dtname", list(DTYPES))
def test_wgrad_repeats_bit_for_bit(A, dtname, k, cin, cout):
    runs, _ = _wgrad_runs(A, dtname, k, cin, cout)
    bad_w, bad_b, ratio = _wgrad_verdict(dtname, k, cin, cout, runs)
    worst = max(float((dw.double() - runs[0][0].double()).abs().max()) for dw, _ in runs)
    print(f"wgrad {dtname} {k}x{k} {cin}->{cout}: runs differing from run 1: dw {bad_w} db {bad_b}; largest |dw - dw1| {worst:.3e}; error / bound {ratio:.3f}")
    assert not bad_w, f"dw of runs {bad_w} (of {RUNS}) differs in its bits from run 1 (largest difference {worst:.3e})"
    assert not bad_b, f"db of runs {bad_b} (of {RUNS}) differs in its bits from run 1"
    assert ratio <= 1.0, f"run 1 against float64: {ratio:.3f} of the bound 1e-4 * max|ref|"


_CHILD = {}


def _wgrad_child():
    if "result" in _CHILD:
        return _CHILD["result"]
    if "failed" in _CHILD:
        pytest.fail(_CHILD["failed"])
    cmd = [sys.executable, os.path.abspath(__file__), "wgrad-child"]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, env=D.child_env("SRK_NO_WS"), timeout=CHILD_TIMEOUT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _CHILD["failed"] = f"the SRK_NO_WS child ran into its time limit of {CHILD_TIMEOUT} s"
        pytest.fail(_CHILD["failed"])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        _CHILD["failed"] = f"the SRK_NO_WS child ended with status {p.returncode}: {p.stderr[-3000:]}"      # runs once: nothing is retried
        pytest.fail(_CHILD["failed"])
    _CHILD["result"] = json.loads(lines[-1][7:])
    return _CHILD["result"]


@pytest.mark.parametrize("k,cin,cout", WGRAD_SHAPES, ids=[f"{k}x{k}-{ci}to{co}" for k, ci, co in WGRAD_SHAPES])
@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
def test_wgrad_fallback_repeats_bit_for_bit(dtname, k, cin, cout):
    """The 16-bit shapes through the generic kernel (SRK_NO_WS=1, one child for all cases)."""
    c = _wgrad_child()[f"{dtname}/{k}/{cin}/{cout}"]
    assert not c["bad_w"], f"dw of runs {c['bad_w']} (of {RUNS}) differs in its bits from run 1"
    assert not c["bad_b"], f"db of runs {c['bad_b']} (of {RUNS}) differs in its bits from run 1"
    assert c["ratio"] <= 1.0, f"run 1 against float64: {c['ratio']:.3f} of the bound 1e-4 * max|ref|"
    assert c["kernels"] == [f"wgrad_generic<{k}>"] * RUNS, f"the knob did not move the launch: {c['kernels']}"


def _run_wgrad_child():
    sys.path.insert(0, ROOT)
    import sr_amd as A
    assert torch.cuda.is_available()
    out = {}
    with D.Recorder() as R:
        for dtname in ("bf16", "fp16"):
            for k, cin, cout in WGRAD_SHAPES:
                runs, names = _wgrad_runs(A, dtname, k, cin, cout, recorder=R)
                bad_w, bad_b, ratio = _wgrad_verdict(dtname, k, cin, cout, runs)
                out[f"{dtname}/{k}/{cin}/{cout}"] = dict(bad_w=bad_w, bad_b=bad_b, ratio=ratio, kernels=names)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. forward + loss + backward of every model
# ---------------------------------------------------------------------------------------------------------------------------------------
def _smallest(cls, **match):
    """kwargs of the smallest configuration of `cls` in tests/golden/manifest.json (what tests/test_gpu_models.py builds)."""
    ents = [v for v in MANIFEST.values() if v["class"] == cls and all(v["kwargs"].get(a) == b for a, b in match.items())]
    return dict(min(ents, key=lambda v: v["n_params_trainable"])["kwargs"])


# the smallest scale factor each model takes is 2 (the smallest WDSR-A of the manifest is a x4 net: same net, x2)
MODELS = {"DDBPN": ("DDBPN", _smallest("DDBPN")), "EDSR": ("EDSR", _smallest("EDSR")), "RCAN": ("RCAN", _smallest("RCAN")),
          "RDN": ("RDN", _smallest("RDN")), "SRCNN": ("SRCNN", _smallest("SRCNN")), "SRResNet": ("SRResNet", _smallest("SRResNet")),
          "WDSR-A": ("WDSR", dict(_smallest("WDSR", type="A"), scale_factor=2)), "WDSR-B": ("WDSR", _smallest("WDSR", type="B"))}


def test_every_model_class_is_covered(A):
    assert sorted({cls for cls, _ in MODELS.values()} | {"SRModel"}) == sorted(A.models.__all__)
    assert all(kw["scale_factor"] == 2 for _, kw in MODELS.values())


@pytest.mark.parametrize("precision", [32, 16, "bf16"])
@pytest.mark.parametrize("model", list(MODELS))
def test_backward_repeats_bit_for_bit(A, model, precision):
    from sr_amd import trainer as T
    cls, kw = MODELS[model]
    torch.manual_seed(0)
    m = getattr(A, cls)(precision=precision, losses="l1", **kw).cuda()
    batch = T.synthetic_batch(8, 3, 24, kw["scale_factor"], 900, "cuda")
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    runs = []
    for _ in range(RUNS):
        for p in m.parameters():
            p.grad = None
        sr = m(batch["lr"])
        loss = m._calculate_losses(img_sr=sr, img_hr=batch["hr"])["loss"]
        loss.backward()
        torch.cuda.synchronize()
        params = dict(m.named_parameters())
        assert all(params[k].grad is not None for k in names)
        runs.append((sr.detach().clone(), loss.detach().clone(), {k: params[k].grad.detach().clone() for k in names}))
    sr1, loss1, g1 = runs[0]
    assert len(names) >= 6 and torch.isfinite(loss1) and any(float(g.abs().max()) > 0 for g in g1.values())
    for i, (sr, loss, g) in enumerate(runs[1:], 2):
        assert same_bits(sr, sr1), f"{model} {precision}: the forward pass of run {i} differs from run 1"
        assert same_bits(loss, loss1), f"{model} {precision}: the loss of run {i} differs from run 1 ({float(loss)!r} / {float(loss1)!r})"
        diff = [k for k in names if not same_bits(g[k], g1[k])]
        assert not diff, (f"{model} {precision}: run {i} differs from run 1 in the gradient of {diff[0]} {tuple(g1[diff[0]].shape)} "
                          f"(by up to {float((g[diff[0]] - g1[diff[0]]).abs().max()):.3e}) and of {len(diff) - 1} more of {len(names)} parameters: {diff[1:8]}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. Trainer.fit: eager twice, then replayed
# ---------------------------------------------------------------------------------------------------------------------------------------
FIT_MODELS = {"EDSR": ("EDSR", dict(scale_factor=2, n_feats=32, n_resblocks=2, res_scale=0.1)), "RCAN": ("RCAN", _smallest("RCAN"))}
FIT_STEPS = 6


def _fit(A, model, precision, use_graph):
    from sr_amd import trainer as T
    cls, kw = FIT_MODELS[model]
    torch.manual_seed(0)
    m = getattr(A, cls)(precision=precision, losses="l1", optimizer="ADAM", **kw)
    tr = T.Trainer(device="cuda", use_graph=use_graph)
    tr.fit(m, (T.synthetic_batch(8, 3, 24, 2, 700 + i, "cpu") for i in range(FIT_STEPS)))
    torch.cuda.synchronize()
    return tr, {k: p.detach().clone() for k, p in m.named_parameters()}


def _assert_same_fit(what, a, b):
    (ta, pa), (tb, pb) = a, b
    la, lb = ta.losses, tb.losses
    assert len(la) == len(lb) == FIT_STEPS and all(np.isfinite(la)), (la, lb)
    assert _float_bits(la) == _float_bits(lb), f"{what}: the losses part at step {[x == y for x, y in zip(_float_bits(la), _float_bits(lb))].index(False) + 1}: {la} / {lb}"
    assert list(pa) == list(pb)
    diff = [k for k in pa if not same_bits(pa[k], pb[k])]
    assert not diff, (f"{what}: after {FIT_STEPS} steps {len(diff)} of {len(pa)} parameters differ, first {diff[0]} "
                      f"(by up to {float((pa[diff[0]] - pb[diff[0]]).abs().max()):.3e})")


@pytest.mark.parametrize("precision", [32, "bf16", 16])
@pytest.mark.parametrize("model", list(FIT_MODELS))
def test_fit_repeats_and_replays_bit_for_bit(A, model, precision):
    """fp16 runs under the device loss scaler, whose launches are part of the captured step: it is held to the same equality."""
    eager, again, graph = _fit(A, model, precision, False), _fit(A, model, precision, False), _fit(A, model, precision, True)
    g = graph[0].graphed
    assert g is not None and g.graphs is not None and not g.failed, "the step was captured"
    assert eager[0].graphed is None
    torch.manual_seed(0)
    fresh = getattr(A, FIT_MODELS[model][0])(precision=precision, losses="l1", optimizer="ADAM", **FIT_MODELS[model][1])
    moved = [k for k, p in fresh.named_parameters() if p.requires_grad and not same_bits(p.detach().cuda(), eager[1][k])]
    assert len(moved) >= 6, f"the training moved the weights: {moved}"
    _assert_same_fit(f"{model} {precision}: two eager runs", eager, again)
    _assert_same_fit(f"{model} {precision}: replayed against eager", graph, eager)


if __name__ == "__main__":
    assert sys.argv[1:] == ["wgrad-child"], sys.argv
    print("RESULT " + json.dumps(_run_wgrad_child()))
