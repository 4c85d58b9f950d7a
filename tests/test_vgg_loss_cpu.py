"""The VGG perceptual loss without a GPU: the torch path of sr_amd.vgg_loss against the float64 statement of tests/vgg_ref.py, gradcheck,
the parameter parser and its refusals, the weight files it takes and refuses, the model's loss table, train.py, the re-exports and the
C ABI.  The weights are seeded random ones (tests/vgg_ref.py): nothing is downloaded, here or in the code under test."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vgg_ref as REF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE_IDS = ["x".join(map(str, s)) for s in REF.SHAPES]
NL_IDS = [f"{n}-{l}" for n, l in REF.NETS_LAYERS]


@pytest.fixture(scope="module")
def V():
    from sr_amd import vgg_loss
    return vgg_loss


def _features(V, net, layer):
    return V.VGGFeatures(REF.weights(net, layer), net, layer)


@pytest.fixture()
def weights_file(tmp_path):
    """A relu5_4-deep vgg19 `features` state dict of the seeded test weights, in a file."""
    path = tmp_path / "vgg19_features.pth"
    torch.save(REF.weights("vgg19", "relu5_4"), path)
    return str(path)


@pytest.mark.parametrize("shape", REF.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("net,layer", REF.NETS_LAYERS, ids=NL_IDS)
def test_torch_path_is_the_float64_statement(V, net, layer, shape):
    ref = REF.reference(net, layer, shape)
    frac = REF.active_fraction(ref["fs"])
    assert 0.25 <= frac <= 0.75, f"the test weights leave {frac:.2f} of the features active: a dead (or all-pass) stack proves nothing"
    sr, hr = REF.images(shape)
    feats = _features(V, net, layer)
    f = V.vgg_features(sr.double(), feats)
    assert f.dtype == torch.float64 and REF.rel(f, ref["fs"]) <= 1e-12
    for crit in REF.CRITERIA:
        s = sr.double().requires_grad_(True)
        loss = V.vgg_loss_torch(s, hr.double(), feats, rescale=REF.RESCALE, criterion=crit)
        loss.backward()
        want, gwant = ref[crit]
        loss = loss.detach()
        assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want)), (crit, float(loss), float(want))
        assert REF.rel(s.grad, gwant) <= 1e-12, (crit, REF.rel(s.grad, gwant))
        assert float(V.vgg_loss(sr.double(), hr.double(), feats, REF.RESCALE, crit)) == float(loss)      # CPU tensors take this path


@pytest.mark.parametrize("criterion", REF.CRITERIA)
def test_gradcheck(V, criterion):
    """(l1 is not differentiable where the features coincide: sr != hr.)"""
    feats = _features(V, "vgg19", "relu2_2")
    sr, hr = REF.make_images((1, 3, 16, 16), 7)
    s = sr.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: V.vgg_loss_torch(x, hr.double(), feats, rescale=1.0, criterion=criterion), (s,),
                                    eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)


def test_hr_receives_no_gradient_through_the_entry(V):
    feats = _features(V, "vgg16", "relu2_2")
    sr, hr = REF.images((2, 3, 16, 16))
    s, h = sr.clone().requires_grad_(True), hr.clone()
    V.vgg_loss(s, h, feats).backward()
    assert s.grad is not None and s.grad.abs().sum() > 0 and h.grad is None
    # the fp32 torch path agrees with the float64 statement to fp32 accuracy
    assert abs(float(V.vgg_loss(sr, hr, feats)) - float(REF.reference("vgg16", "relu2_2", (2, 3, 16, 16))["l2"][0])) <= 1e-5 * float(
        REF.reference("vgg16", "relu2_2", (2, 3, 16, 16))["l2"][0])


def test_shapes_are_checked_at_call_time(V):
    feats = _features(V, "vgg19", "relu5_4")
    assert feats.pools == 4 and feats.min_size == 16
    x = torch.rand(1, 3, 15, 16)
    with pytest.raises(ValueError, match="at least 16"):
        V.vgg_loss(x, x, feats)
    with pytest.raises(ValueError, match="at least 16"):
        V.vgg_features(x, feats)
    with pytest.raises(ValueError, match="3 channels"):
        V.vgg_loss(torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16), feats)
    with pytest.raises(ValueError, match="one shape"):
        V.vgg_loss(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 18), feats)
    with pytest.raises(ValueError, match="criterion"):
        V.vgg_loss(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16), feats, criterion="huber")


# ---- the parser ----------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_tolerance(V):
    p = V.vgg_loss_parse_params(["vgg.weights=/some/Dir/w.pth"])
    assert p == {"weights": "/some/Dir/w.pth", "net": "vgg19", "layer": "relu2_2", "rescale": 0.006, "criterion": "l2", "dtype": torch.float32}
    assert V.vgg_loss_parse_params(["vgg.weights=w"], torch.bfloat16)["dtype"] is torch.bfloat16
    p = V.vgg_loss_parse_params([" VGG.Weights = /A b/W.pth ", "vgg.NET= VGG16 ", " vgg.layer =ReLU4_3", "vgg.rescale = 1e-2", "Vgg.criterion=L1",
                                 "vgg.precision = BF16 "], torch.float16)
    assert p == {"weights": "/A b/W.pth", "net": "vgg16", "layer": "relu4_3", "rescale": 0.01, "criterion": "l1", "dtype": torch.bfloat16}
    assert [V.vgg_loss_parse_params(["vgg.weights=w", f"vgg.precision={s}"])["dtype"] for s in ("32", "16", "bf16")] == \
        [torch.float32, torch.float16, torch.bfloat16]


@pytest.mark.parametrize("entries,match", [
    (["vgg.weights=w", "vgg.depth=3"], "has no parameter depth"),
    (["vgg.weights=w", "vggweights"], "is not vgg.<key>=<value>"),
    (["vgg.weights=w", "vgg.layer="], "is not vgg.<key>=<value>"),
    (["vgg.weights=w", "ffl.alpha=1"], "is not vgg.<key>=<value>"),
    (["vgg.weights=w", "vgg.net=vgg11"], "net='vgg11' is not recognized"),
    (["vgg.weights=w", "vgg.criterion=huber"], "criterion='huber' is not recognized"),
    (["vgg.weights=w", "vgg.precision=8"], "precision='8' is not recognized"),
    (["vgg.weights=w", "vgg.rescale=big"], "rescale='big' is not a float"),
    (["vgg.weights=w", "vgg.rescale=inf"], "out of range"),
    (["vgg.weights=w", "vgg.layer=relu3_3"], "vgg19 has no layer 'relu3_3'"),
    (["vgg.weights=w", "vgg.net=vgg16", "vgg.layer=relu5_4"], "vgg16 has no layer 'relu5_4'"),
    (["vgg.weights=w", "vgg.layer=conv1_1"], "has no layer"),
    (["vgg.layer=relu2_2"], "needs weights"),
    ([], "needs weights"),
])
def test_parser_refusals(V, entries, match):
    with pytest.raises(ValueError, match=re.escape(match)):
        V.vgg_loss_parse_params(entries)


# ---- weight files ---------------------------------------------------------------------------------------------------------------
def test_both_key_layouts_load_and_classifier_is_ignored(V, tmp_path):
    bare = REF.weights("vgg19", "relu3_4")
    full = {f"features.{k}": v for k, v in bare.items()}
    full.update({"classifier.0.weight": torch.zeros(4, 4), "classifier.0.bias": torch.zeros(4)})
    torch.save(bare, tmp_path / "bare.pth")
    torch.save(full, tmp_path / "full.pth")
    sr, _ = REF.images((2, 3, 16, 16))
    want = V.vgg_features(sr, V.VGGFeatures(bare, "vgg19", "relu3_4"))
    for w in (str(tmp_path / "bare.pth"), str(tmp_path / "full.pth"), tmp_path / "full.pth", full):
        feats = V.VGGFeatures(w, "vgg19", "relu3_4")
        assert len(feats.convs) == 8 and torch.equal(V.vgg_features(sr, feats), want)
    # only the layers up to the slice are kept: a deeper file serves a shallower slice, and what lies behind it is not read
    deep = dict(REF.weights("vgg19", "relu5_4"))
    deep["34.weight"] = torch.zeros(1)
    assert len(V.VGGFeatures(deep, "vgg19", "relu2_2").convs) == 4


def test_bad_weight_files_are_refused(V, tmp_path):
    bare = REF.weights("vgg19", "relu3_4")
    missing = {k: v for k, v in bare.items() if k != "12.bias"}
    with pytest.raises(ValueError, match="have no '12.bias'"):
        V.VGGFeatures(missing, "vgg19", "relu3_4")
    with pytest.raises(ValueError, match=re.escape("have no 'features.16.weight'")):
        V.VGGFeatures({f"features.{k}": v for k, v in bare.items() if not k.startswith("16.")}, "vgg19", "relu3_4")
    wrong = dict(bare)
    wrong["5.weight"] = torch.zeros(128, 64, 5, 5)
    with pytest.raises(ValueError, match=re.escape("'5.weight' has shape (128, 64, 5, 5), vgg19 needs (128, 64, 3, 3)")):
        V.VGGFeatures(wrong, "vgg19", "relu3_4")
    # the other net's file: vgg16 has convs at features 17, 24, 26 and none at 16, 23, 25, ...
    v16 = REF.weights("vgg16", "relu4_3")
    with pytest.raises(ValueError, match="look like vgg16's"):
        V.VGGFeatures(v16, "vgg19", "relu4_4")
    with pytest.raises(ValueError, match="look like vgg16's"):
        V.VGGFeatures(v16, "vgg19", "relu2_2")
    with pytest.raises(ValueError, match="look like vgg19's"):
        V.VGGFeatures({f"features.{k}": v for k, v in REF.weights("vgg19", "relu5_4").items()}, "vgg16", "relu4_3")
    torch.save([1, 2, 3], tmp_path / "list.pth")
    with pytest.raises(ValueError, match="not a state dict"):
        V.VGGFeatures(str(tmp_path / "list.pth"))
    with pytest.raises(ValueError, match="has no layer"):
        V.VGGFeatures(bare, "vgg16", "relu3_4")


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_model_refusals(weights_file):
    import sr_amd
    with pytest.raises(ValueError, match="needs weights"):
        sr_amd.SRCNN(scale_factor=2, losses="l1+0.006*vgg")
    with pytest.raises(ValueError, match="channels == 3"):
        sr_amd.SRCNN(channels=1, scale_factor=2, losses="vgg", loss_params=[f"vgg.weights={weights_file}"])
    with pytest.raises(ValueError, match="channels == 3"):
        sr_amd.SRCNN(channels=1, scale_factor=2, losses="vgg")
    with pytest.raises(ValueError, match="HR patch of at least 16"):
        sr_amd.SRCNN(scale_factor=2, patch_size=8, losses="vgg", loss_params=[f"vgg.weights={weights_file}", "vgg.layer=relu5_4"])
    with pytest.raises(ValueError, match="has no parameter depth"):
        sr_amd.SRCNN(scale_factor=2, losses="vgg", loss_params=[f"vgg.weights={weights_file}", "vgg.depth=2"])
    short = os.path.join(os.path.dirname(weights_file), "short.pth")          # a file that ends before the layer
    torch.save(REF.weights("vgg19", "relu4_4"), short)
    with pytest.raises(ValueError, match="have no '28.weight'"):
        sr_amd.SRCNN(scale_factor=2, losses="vgg", loss_params=[f"vgg.weights={short}", "vgg.layer=relu5_4"])
    # a vgg entry without vgg among the losses stays refused where such entries always were
    with pytest.raises(ValueError, match="is not among the losses"):
        sr_amd.SRCNN(scale_factor=2, losses="l1", loss_params=[f"vgg.weights={weights_file}"])


def test_model_is_unchanged_by_the_term(V, weights_file):
    import sr_amd
    torch.manual_seed(0)
    plain = sr_amd.SRCNN(scale_factor=2, losses="l1")
    torch.manual_seed(0)
    m = sr_amd.SRCNN(scale_factor=2, losses="0.5*l1+0.006*vgg", loss_params=[f" VGG.weights = {weights_file} ", "vgg.layer=relu3_4"], precision="bf16")
    assert list(m.state_dict()) == list(plain.state_dict())
    assert [tuple(p.shape) for p in m.parameters()] == [tuple(p.shape) for p in plain.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), plain.parameters()))
    assert [n for n, _ in m.named_modules()] == [n for n, _ in plain.named_modules()]
    term = m._losses[1].loss
    assert isinstance(term, V.VGGLoss) and not isinstance(term, torch.nn.Module) and callable(term)
    assert (term.features.net, term.features.layer, term.rescale, term.criterion, term.dtype) == ("vgg19", "relu3_4", 0.006, "l2", torch.bfloat16)
    assert len(term.features.convs) == 8 and term.features._packs == {}            # loaded at construction, packed on the first GPU call
    assert len(list(m.configure_optimizers()[0].param_groups[0]["params"])) == len(list(plain.parameters()))


def test_composite_on_cpu_tensors(V, weights_file):
    import sr_amd
    m = sr_amd.SRCNN(scale_factor=2, losses="0.5*l1+0.006*vgg", loss_params=[f"vgg.weights={weights_file}"])
    assert [(l.name, l.weight) for l in m._losses] == [("l1", 0.5), ("vgg", 0.006)]
    g = torch.Generator().manual_seed(0)
    lr, hr = torch.rand(2, 3, 8, 8, generator=g), torch.rand(2, 3, 16, 16, generator=g)
    out = m.training_step({"lr": lr, "hr": hr}, 0)
    assert set(out) == {"loss/l1", "loss/vgg", "loss"}
    sr = m(lr).detach()
    feats = V.VGGFeatures(REF.weights("vgg19", "relu2_2"), "vgg19", "relu2_2")
    want = 0.006 * float(REF.loss(sr, hr, REF.weights("vgg19", "relu2_2"), "vgg19", "relu2_2", rescale=0.006))
    assert abs(float(out["loss/vgg"]) - want) <= 1e-5 * want
    assert abs(float(out["loss/vgg"]) - 0.006 * float(V.vgg_loss_torch(sr, hr, feats))) <= 1e-6 * want
    assert torch.allclose(out["loss"], out["loss/l1"] + out["loss/vgg"])
    out["loss"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_loss_tables(V):
    from sr_amd.models import srmodel
    names = list(srmodel._supported_losses)
    assert names[-2:] == ["fft", "ffl"] and names[-3] == "vgg"
    assert srmodel._out_of_scope_losses == {"adaptive", "dists", "edge_loss", "lpips", "pencil_sketch", "pieapp"}


def test_train_py_takes_the_strings():
    sys.path.insert(0, ROOT)
    import train
    a = train.parse(["--losses", "l1+0.006*vgg", "--loss_params", "vgg.weights=/w/vgg19.pth", "vgg.layer=relu5_4", "vgg.criterion=l1"])
    assert a.losses == "l1+0.006*vgg" and a.loss_params == ["vgg.weights=/w/vgg19.pth", "vgg.layer=relu5_4", "vgg.criterion=l1"]


def test_ops_reexports():
    import sr_amd
    for name in ("VGGFeatures", "vgg_loss", "vgg_features", "vgg_loss_torch", "VGGLossFn", "vgg_loss_parse_params", "VGGLoss"):
        assert hasattr(sr_amd.ops, name), name


def test_args_mirror_the_header():
    import sr_amd
    L = sr_amd._lib
    assert L.LAUNCHERS["srk_vgg_prepare"] is L.VggPrepareArgs and L.LAUNCHERS["srk_vgg_image_grad"] is L.VggImageGradArgs
    assert all(L.LAUNCHERS[f"srk_vgg_pool_{k}"] is L.VggPoolArgs for k in ("fwd", "bwd"))
    assert all(L.LAUNCHERS[f"srk_vgg_feat_{k}"] is L.VggFeatArgs for k in ("fwd", "finalize", "grad"))
    assert "srk_vgg_blocks" in L.OTHER_SYMBOLS and (L.SRK_VGG_L2, L.SRK_VGG_L1) == (0, 1)


def test_block_counts_of_the_library():
    """Host code: one workgroup of 256 lanes per 256 chunks, at least one, at most SRK_VGG_BLOCKS_MAX."""
    import sr_amd
    b = sr_amd._lib.load().srk_vgg_blocks
    assert [b(n) for n in (0, 1, 256, 257, 2048 * 256, 2048 * 256 + 1, 1 << 40)] == [1, 1, 1, 2, 2048, 2048, 2048]
    assert sr_amd._lib.SRK_VGG_BLOCKS_MAX == 2048


def test_hip_entries_refuse_the_cpu(V):
    feats = _features(V, "vgg19", "relu1_2")
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.VGGLossFn.apply(x, x, feats, 0.006, "l2", torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.max_pool_nhwc(torch.rand(1, 4, 4, 16))


def test_documented_numbers_follow_from_the_profile_file():
    """INTEGRATION.md's "VGG perceptual loss" tables are generated from profiles/vgg_loss.txt (tools/gen_results.py vgg_loss), which holds
    the measured timings of both layers and an error line per (net, layer, storage dtype)."""
    import json
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_results.py"), "vgg_loss", "--check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    with open(os.path.join(ROOT, "profiles", "vgg_loss.txt")) as f:
        rows = [json.loads(line) for line in f if line.startswith("{")]
    timed = [r for r in rows if "hip_fwd_bwd_us" in r]
    assert {r["layer"] for r in timed} == {"relu2_2", "relu5_4"} and all(r["shape"] == "16x3x192x192" and r["hip_fwd_bwd_us"] > 0 for r in timed)
    assert all("ratio_faster_eager_over_hip" in r for r in timed)
    assert {(r["errors"], r["dtype"]) for r in rows if "errors" in r} == {(f"{n} {l}", d) for n, l in REF.NETS_LAYERS for d in ("fp32", "bf16", "fp16")}
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert "VGG perceptual loss" in text and f"{timed[0]['hip_fwd_bwd_us']:,.0f}" in text


def test_nothing_downloads():
    """No torchvision `pretrained` constructor, no URL and no unconditional torchvision import in the new Python sources."""
    for rel in ("sr-pytorch-lightning_amd/vgg_loss.py", "tools/microbench_vgg_loss.py"):
        with open(os.path.join(ROOT, rel)) as f:
            text = f.read()
        assert "pretrained" not in text.lower(), rel
        assert not re.search(r"https?://|ftp://|urllib|requests\.|load_state_dict_from_url|hub\.load", text), rel
        assert not re.search(r"^\s*(import|from)\s+torchvision", text, flags=re.M), rel
