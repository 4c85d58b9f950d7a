"""The exponential moving average of the weights (sr_amd.ema.ParamEMA) where no GPU is needed: the CPU form of the recurrence against
the float64 restatement (tests/ema_ref.py), argument checks, the swap, the state-dict round trip through train.py --save and
predict.py --weights, and Trainer.fit on SRCNN."""
import copy
import importlib.util
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ema_ref import EmaRef  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (3,), (5,), (4097,), (16, 8, 3, 3), (33, 100)]


@pytest.fixture(scope="module")
def A():
    import sr_amd
    return sr_amd


def _params(seed, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.rand(*s, generator=g) - 0.5) for s in shapes]


def _move(ps, step):
    """The parameters change by about 0.1 (uniform in +-0.1) per step."""
    g = torch.Generator().manual_seed(500 + step)
    with torch.no_grad():
        for p in ps:
            p.add_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)


def _np(ts):
    return [t.detach().double().numpy() for t in ts]


@pytest.mark.parametrize("decay", [0.9, 0.999, 0.3])
def test_cpu_update_matches_the_restatement(A, decay):
    ps = _params(1)
    frozen = ps[2].requires_grad_(False)                      # averaged like the trainable ones
    ema = A.ema.ParamEMA(ps, decay)
    assert not ema.on_gpu and ema.num_updates == 0
    for p in ps:
        assert torch.equal(ema.shadow(p), p.detach()) and ema.shadow(p).shape == p.shape
    ref = EmaRef(_np(ps), decay)
    for step in range(20):
        _move(ps, step)
        ema.update()
        ref.update(_np(ps))
    assert ema.num_updates == ref.count == 20
    bound = ref.bound()
    worst = max(float(np.abs(ema.shadow(p).double().numpy() - s).max()) for p, s in zip(ps, ref.s))
    print("decay %g: max |err| %.3e (bound %.3e)" % (decay, worst, bound))
    assert worst <= bound
    assert not torch.equal(ema.shadow(frozen), frozen)


def test_decay_is_validated(A):
    ps = _params(2, [(4,)])
    for bad in (-0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            A.ema.ParamEMA(ps, bad)
        with pytest.raises(ValueError):
            A.SRCNN(ema_decay=bad)
    ema = A.ema.ParamEMA(ps, 0.0)
    ema.set_decay(1.0)
    with pytest.raises(ValueError):
        ema.set_decay(2.0)
    assert ema.decay == 1.0
    with pytest.raises(ValueError):
        A.ema.ParamEMA([torch.zeros(3, dtype=torch.int64)], 0.9)      # nothing floating point to average


def test_ema_off_allocates_nothing(A):
    m = A.SRCNN(scale_factor=2)
    assert m.ema_decay == 0.0 and m.ema is None and "ema" not in m.__dict__
    before = copy.deepcopy(m.state_dict())
    with m.ema_weights() as ctx:
        assert ctx is None
    from sr_amd import trainer as T
    T.Trainer(device="cpu", max_steps=2).fit(m, (T.synthetic_batch(2, 3, 8, 2, s, "cpu") for s in range(2)))
    assert m.ema is None
    assert list(m.state_dict()) == list(before)               # no buffer appeared


def test_swapped_restores_every_bit_also_when_the_body_raises(A):
    ps = _params(3)
    ema = A.ema.ParamEMA(ps, 0.5)
    _move(ps, 0)
    ema.update()
    live = [p.detach().clone() for p in ps]
    avg = [ema.shadow(p).clone() for p in ps]
    vers = [p._version for p in ps]
    with ema.swapped():
        for p, a, l in zip(ps, avg, live):
            assert torch.equal(p.detach(), a) and torch.equal(ema.shadow(p), l)
        assert all(p._version > v for p, v in zip(ps, vers))
    with pytest.raises(KeyError):
        with ema.swapped():
            raise KeyError("body")
    for p, a, l in zip(ps, avg, live):
        assert torch.equal(p.detach(), l) and torch.equal(ema.shadow(p), a)
    ema.load()
    for p, a in zip(ps, avg):
        assert torch.equal(p.detach(), a)
    _move(ps, 1)
    ema.store()
    for p in ps:
        assert torch.equal(ema.shadow(p), p.detach())


def test_state_dict_round_trip_and_module_copies(A):
    torch.manual_seed(0)
    m = A.SRCNN(scale_factor=2, ema_decay=0.9)
    ema = m.make_ema()
    _move(list(m.parameters()), 0)
    ema.update()
    ema.update()
    sd = ema.state_dict(m)
    assert list(sd) == list(m.state_dict()) and sd.num_updates == 2
    for k, p in m.named_parameters():
        assert torch.equal(sd[k], ema.shadow(p)) and not torch.equal(sd[k], p.detach())
    fresh = A.SRCNN(scale_factor=2)
    fresh.load_state_dict(sd, strict=True)                    # a plain load accepts it
    # the inverse, into another average
    other = A.SRCNN(scale_factor=2, ema_decay=0.5)
    e2 = other.make_ema()
    e2.load_state_dict(other, sd)
    assert e2.num_updates == 2
    for (k, p), (_, q) in zip(m.named_parameters(), other.named_parameters()):
        assert torch.equal(e2.shadow(q), ema.shadow(p))
    # SRModel.state_dict() is the reference's layout; copies and pickles of the module start without an average
    assert not any("ema" in k for k in m.state_dict())
    assert copy.deepcopy(m).ema is None and pickle.loads(pickle.dumps(m)).ema is None and m.ema is ema


def _script(name):
    spec = importlib.util.spec_from_file_location("_ema_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_save_and_predict_weights(A, tmp_path):
    """train.py --ema_decay --save writes both sets of weights and the count; --checkpoint restores the shadow; predict.py --weights
    picks the set, `auto` the averaged one, and a file from before this option loads as it did."""
    from PIL import Image
    train, predict = _script("train"), _script("predict")
    ck, ck2, old = tmp_path / "m.pt", tmp_path / "m2.pt", tmp_path / "old.pt"
    common = ["-m", "srcnn", "-s", "2", "--patch_size", "16", "--batch_size", "2", "--accelerator", "cpu", "--precision", "32", "--log_every", "0"]
    train.main(common + ["--max_steps", "3", "--ema_decay", "0.5", "--save", str(ck)])
    f = torch.load(ck)
    assert set(f) == {"state_dict", "state_dict_ema", "ema_num_updates"} and f["ema_num_updates"] == 3
    assert list(f["state_dict"]) == list(f["state_dict_ema"])
    assert any(not torch.equal(f["state_dict"][k], f["state_dict_ema"][k]) for k in f["state_dict"])
    # resumed: the shadow and the count continue from the file (decay 1 keeps the shadow where it was)
    train.main(common + ["--max_steps", "2", "--ema_decay", "1.0", "--checkpoint", str(ck), "--save", str(ck2)])
    f2 = torch.load(ck2)
    assert f2["ema_num_updates"] == 5
    for k in f["state_dict_ema"]:
        assert torch.equal(f2["state_dict_ema"][k], f["state_dict_ema"][k]), k
    assert any(not torch.equal(f2["state_dict"][k], f["state_dict"][k]) for k in f["state_dict"])
    # a checkpoint without an average: the shadow starts from the loaded weights
    torch.save({"state_dict": f["state_dict"]}, old)
    train.main(common + ["--max_steps", "0", "--ema_decay", "0.9", "--checkpoint", str(old), "--save", str(ck2)])
    f3 = torch.load(ck2)
    assert f3["ema_num_updates"] == 0 and all(torch.equal(f3["state_dict_ema"][k], f["state_dict"][k]) for k in f["state_dict"])

    lr_dir = tmp_path / "Set5"
    lr_dir.mkdir()
    img = np.random.default_rng(0).integers(0, 255, (20, 24, 3), dtype=np.uint8)
    Image.fromarray(img).save(lr_dir / "a.png")
    x = torch.from_numpy(img.copy()).permute(2, 0, 1).float()[None] / 255.0

    def want(sd):
        m = A.SRCNN(scale_factor=2, precision=32)
        m.load_state_dict(sd)
        with torch.no_grad():
            return A.SRModel.to_uint8(m(x).clamp(0, 1)[0]).permute(1, 2, 0).numpy()

    def got(path, *extra):
        res = tmp_path / ("res_" + "_".join(extra).strip("-") + os.path.basename(str(path)))
        predict.main(["-m", "srcnn", "-s", "2", "--checkpoint", str(path), "--predict_datasets", str(lr_dir), "--default_root_dir", str(res),
                      "--accelerator", "cpu", "--precision", "32"] + list(extra))
        return np.asarray(Image.open(res / "Set5" / "a.png"))

    w_live, w_ema = want(f["state_dict"]), want(f["state_dict_ema"])
    assert not np.array_equal(w_live, w_ema)
    assert np.array_equal(got(ck), w_ema)
    assert np.array_equal(got(ck, "--weights", "ema"), w_ema)
    assert np.array_equal(got(ck, "--weights", "live"), w_live)
    assert np.array_equal(got(old), w_live) and np.array_equal(got(old, "--weights", "live"), w_live)
    with pytest.raises(SystemExit):
        got(old, "--weights", "ema")


@pytest.mark.parametrize("decay", [0.0, 1.0, 0.9])
def test_trainer_fit_cpu_srcnn(A, decay):
    """Six steps: six updates, each behind its optimizer step.  decay 0: the shadow is the final weights bit for bit (the last update
    followed the last step); decay 1: the initial ones."""
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = A.SRCNN(scale_factor=2, precision=32, ema_decay=decay)
    if decay == 0.0:                                          # (`ema_decay=0` is "off": an average made by hand, which fit() adopts)
        m.make_ema(decay=0.0)
    torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])    # torch's own Adam.step is wrapped too from here on: still one update per step
    first = [p.detach().clone() for p in m.parameters()]
    tr = T.Trainer(device="cpu", max_steps=6)
    tr.fit(m, (T.synthetic_batch(2, 3, 8, 2, 40 + s, "cpu") for s in range(8)))
    assert len(tr.losses) == 6 and m.ema.num_updates == 6
    last = [p.detach() for p in m.parameters()]
    assert any(not torch.equal(a, b) for a, b in zip(first, last))
    shadows = [m.ema.shadow(p) for p in m.parameters()]
    if decay == 0.0:
        assert all(torch.equal(s, p) for s, p in zip(shadows, last))
    elif decay == 1.0:
        assert all(torch.equal(s, p) for s, p in zip(shadows, first))
    else:
        assert all(not torch.equal(s, p) for s, p in zip(shadows, last))
    # the hooks are gone: a later step of the same kind of optimizer does not touch the average
    opt = m.configure_optimizers()[0]
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    assert m.ema.num_updates == 6
