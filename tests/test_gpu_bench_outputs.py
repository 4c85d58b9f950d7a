"""bench.py --dump-outputs on the GPU, on every path the timed steps can take: the files hold the LAST TIMED step (its loss is the
line's `loss_after_timed_steps` and equals mean |sr - hr| of the dumped output against the bench's own targets), two runs with the
same arguments dump the same values, and where bench.py cannot reach the timed step's output (the trainer's segmented-overlap step)
no output is dumped at all rather than one of another step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUIET = ["--no-cpu-baseline", "--no-roofline", "--no-other-configs", "--sustain-seconds", "0"]


def _bench(out_dir, *args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "4", "--steps", "3", "--warmup", "2", *QUIET, *args,
                        "--dump-outputs", str(out_dir)], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    names = set(line["dump_outputs"]["shapes"])
    assert names == {f[:-4] for f in os.listdir(out_dir)}
    return line, {n: np.load(out_dir / f"{n}.npy") for n in names}


def _check_training_dump(line, d, with_sr=True):
    from sr_amd import trainer as T
    assert set(d) == ({"loss", "sr", "params", "grads"} if with_sr else {"loss", "params", "grads"})
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in d.values())
    loss = float(d["loss"])
    assert loss == pytest.approx(line["config"]["loss_after_timed_steps"], rel=1e-6)
    if with_sr:
        hr = T.synthetic_batch(4, 3, 48, 4, 1234, "cpu")["hr"].numpy()
        assert d["sr"].shape == hr.shape
        assert float(np.abs(d["sr"].astype(np.float64) - hr).mean()) == pytest.approx(loss, rel=1e-4)
    assert d["params"].shape == d["grads"].shape and np.abs(d["grads"]).max() > 0


def test_dump_is_the_last_timed_step_and_repeats(tmp_path):
    line, d = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["config"]["hip_graph"] == "full"
    _check_training_dump(line, d)
    _, d2 = _bench(tmp_path / "b")
    for n, v in d.items():
        scale = max(1e-12, float(np.abs(v).max()))
        assert float(np.abs(d2[n] - v).max()) <= 1e-3 * scale, n


def test_dump_of_the_eager_step(tmp_path):
    line, d = _bench(tmp_path / "a", "--no-graph")
    assert line["config"]["hip_graph"] is False
    _check_training_dump(line, d)


def test_dump_of_the_optimizer_first_graph(tmp_path):
    """SRK_FORCE_DDP=1 (a one-rank process group): the multi-rank step structure, [optimizer step] + forward + backward in one graph."""
    line, d = _bench(tmp_path / "a", env=dict(SRK_FORCE_DDP="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29733", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert line["config"]["hip_graph"] == "segmented"
    _check_training_dump(line, d)


def test_dump_of_the_segmented_overlap_step_has_no_stale_output(tmp_path):
    """EDSR-large's 172 MB of gradients take the trainer's segmented-overlap step after eight eager steps of bench.py's own: the output
    those eager steps computed must not be dumped as the timed step's."""
    line, d = _bench(tmp_path / "a", "--model", "edsr_large",
                     env=dict(SRK_FORCE_DDP="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29734", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert line["config"]["hip_graph"].startswith("segmented_overlap"), line["config"]["hip_graph"]
    _check_training_dump(line, d, with_sr=False)


def test_dump_of_the_inference_step_is_the_models_output(tmp_path):
    import torch
    import sr_amd
    from oracle import functional as OF
    from sr_amd import trainer as T
    line, d = _bench(tmp_path / "a", "--inference")
    assert set(d) == {"sr"} and d["sr"].dtype == np.float32 and line["config"]["hip_graph"] == "full"
    kw = dict(n_feats=64, n_resblocks=16, res_scale=0.1, scale_factor=4)
    torch.manual_seed(0)                                            # bench.py's weights
    sd = sr_amd.EDSR(precision="bf16", **kw).state_dict()
    lr = T.synthetic_batch(4, 3, 48, 4, 1234, "cpu")["lr"]
    with torch.no_grad():
        y = OF.forward("EDSR", sd, lr, **kw).numpy()
    assert d["sr"].shape == y.shape and float(np.abs(d["sr"] - y).max()) < 5e-2
