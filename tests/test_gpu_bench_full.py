"""bench.py's two kinds of run on the GPU: a plain run prints the headline figure and nothing that takes runs of its own; `--full` adds
the sustained window, the roofline and the CPU baseline behind the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("sustained_ms_per_step", "sustained_value", "roofline", "other_configs", "layerwise_hr_stage", "cpu_baseline")


def _bench(batch, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", str(batch), "--steps", "3", "--warmup", "2", *args],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_headline_only():
    line = _bench(4)
    for k in HEADLINE:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 2 and line["value"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - 4 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    assert not [k for k in FULL_ONLY if k in line]


def test_full_run_adds_the_other_measurements():
    line = _bench(16, "--full", "--sustain-seconds", "0.2")           # (the batch of the committed --model M --batch 16 lines)
    for k in HEADLINE:
        assert k in line, k
    assert line["sustained_ms_per_step"] > 0
    r = line["roofline"]
    assert "error" not in r, r
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = line["cpu_baseline"]
    assert "error" not in c and c["value"] > 0 and c["cores"] >= 1
    assert "error" not in c["parity"], c["parity"]
