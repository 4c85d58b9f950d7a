"""bench.py's contract with the driver (no GPU needed): flags, the JSON line's keys / types (checked on the committed
line of the final tree, profiles/r1_final_bench_default.json), and the refusal to run without an MI355X (no CPU
fallback that would print a number)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_exist():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--batch", "--model", "--dtype", "--inference", "--dump-outputs"):
        assert flag in out.stdout


def test_full_is_an_option_and_the_sustained_window_needs_it():
    """A plain run measures the headline figure only; --sustain-seconds asks for a --full leg and is refused without --full
    rather than ignored."""
    bench = os.path.join(ROOT, "bench.py")
    out = subprocess.run([sys.executable, bench, "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--full" in out.stdout
    out = subprocess.run([sys.executable, bench, "--sustain-seconds", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--full" in out.stderr


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--steps" in out.stderr


def test_dump_outputs_fits_64_mb_with_a_fixed_sample(tmp_path):
    """--dump-outputs at the sizes of the largest default configurations: float32 .npy files under 64 MB in all, `sr` sampled as whole
    images, and the same sample on every call (two builds' dumps line up element for element)."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {"loss": torch.tensor(0.25), "sr": torch.rand(256, 3, 192, 192, generator=g), "params": torch.rand(43_000_000, generator=g),
              "grads": torch.rand(1_400_000, generator=g)}
    shapes = [bench.dump_outputs(str(tmp_path / d), arrays) for d in ("a", "b")]
    assert shapes[0] == shapes[1] and set(shapes[0]) == set(arrays)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) < 64e6
    for name, x in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b), name
    assert np.array_equal(np.load(tmp_path / "a" / "grads.npy"), arrays["grads"].numpy())          # under its share: whole
    sr = np.load(tmp_path / "a" / "sr.npy")
    assert sr.shape[1:] == (3, 192, 192) and 1 <= sr.shape[0] < 256
    full = arrays["sr"].numpy()
    assert sum(np.array_equal(full[i], sr[-1]) for i in range(256)) == 1                         # a sampled row is a whole image


def test_committed_line_has_the_contract_keys():
    line = json.loads(open(os.path.join(ROOT, "profiles", "r1_final_bench_default.json")).readline())
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                 ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(line[k], t), k
    assert line["vs_baseline"] is None and line["scaling"] == "weak" and line["data"] == "synthetic"
    assert "workload" in line["config"] and "model" not in line["config"]
    r = line["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None or r["traffic"] > 0
    c = line["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    # value is whole-job throughput: global batch * steps / time
    assert abs(line["value"] - line["config"]["global_batch"] / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3


def test_round5_line_quotes_the_in_step_roofline():
    """ONE fraction at the top of `roofline`, measured in the step (the trunk's convolutions in a training step's order,
    buffers and autograd mode); the per-flavour isolated timings in a sub-object; the CPU model next to the core count."""
    line = json.loads(open(os.path.join(ROOT, "profiles", "r5_bench_default.json")).readline())
    r = line["roofline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "us_per_launch", "flops_per_launch", "where", "traffic", "in_step", "isolated"):
        assert k in r, k
    for k in ("frac_burst", "step_weighted_frac", "step_weighted_frac_burst", "variants_us"):
        assert k not in r, f"{k} belongs to roofline.isolated"
    assert "IN THE STEP" in r["where"]
    ins, iso = r["in_step"], r["isolated"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and abs(r["frac"] - ins["frac"]) < 1e-3
    assert ins["convs"] == 66 and ins["convs_per_launch"] == 1                      # EDSR-baseline: 2 x (2 x 16 + 1) convolutions of 64 -> 64
    assert abs(ins["flops_per_launch"] - 2.0 * 256 * 48 * 48 * 64 * 64 * 9) < 1.0   # executed = algorithmic FLOPs of one 3x3 64 -> 64 launch
    g = ins["graph_us"]
    assert g["pack"] < g["fwd"] < g["fwd_bwd"] < g["fwd_bwd_wgrad"]
    assert abs(ins["us_per_conv"] - (g["fwd_bwd"] - g["pack"]) / ins["convs"]) < 0.05
    assert iso["frac"] >= r["frac"], "an isolated launch re-reads its own buffers: it cannot be slower than the same launch in the step"
    assert set(iso["variants_us"]) == set(iso["variants_us_burst"]) == set(iso["launches_per_block"])
    c = line["cpu_baseline"]
    assert c["cpu_model"] and c["cores"] >= 1 and c["cores_available"] >= c["cores"]
    # the same kernel family in the committed rocprofv3 step trace of the same box: within 5 % (VERDICT r4 item 3's criterion).  The trunk's
    # 66 launches are the conv_ws launches below 100 us (the one above is the first upsampler stage, 64 -> 256)
    durs = []
    for ln in open(os.path.join(ROOT, "profiles", "r5_step_edsr_baseline_b256.txt")):
        if not ln.startswith("conv_ws_kernel"):
            continue
        parts = ln[64:].split()
        if parts[0].startswith("x"):
            durs += [float(parts[1]) / int(parts[0][1:])] * int(parts[0][1:])
        else:
            durs.append(float(parts[1]))
    durs = [d for d in durs if d < 100.0]
    assert len(durs) == ins["convs"]
    trace_frac = ins["flops_per_launch"] / (sum(durs) / len(durs) * 1e-6) / 1e12 / r["peak"]
    assert abs(trace_frac - r["frac"]) / trace_frac < 0.05, (trace_frac, r["frac"])


def test_round6_line_quotes_the_trunk_launch_and_every_config_has_traffic():
    """the in-step fraction of the trunk's convolutions is >= 0.40 of the MFMA peak with the method unchanged (now two launches of 33
    layers: `convs_per_launch`), it agrees with the committed rocprofv3 step trace of the same box, `traffic` (in-step PMC bytes) is non-null for the default line and
    for every bf16 `other_configs` entry, and the line carries the trained-net PSNR deltas next to the CPU baseline."""
    line = json.loads(open(os.path.join(ROOT, "profiles", "r6_bench_default.json")).readline())
    r = line["roofline"]
    ins = r["in_step"]
    assert "IN THE STEP" in r["where"] and "conv_trunk_kernel" in r["kernel"]
    assert ins["convs"] == 66 and ins["convs_per_launch"] == 33 and ins["launch"] == "conv_trunk_kernel"
    assert abs(ins["flops_per_launch"] - 33 * 2.0 * 256 * 48 * 48 * 64 * 64 * 9) < 1.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and abs(r["frac"] - ins["frac"]) < 1e-3
    assert r["frac"] >= 0.40, r["frac"]                                              # north_star: >= 40 % of the MFMA peak on the EDSR-baseline 3x3 conv
    g = ins["graph_us"]
    assert abs(ins["us_per_conv"] - (g["fwd_bwd"] - g["pack"]) / ins["convs"]) < 0.05
    assert r["traffic"] and r["algorithmic_bytes_per_launch"] and 0.95 < r["traffic"] / r["algorithmic_bytes_per_launch"] < 1.15, (r["traffic"], r["algorithmic_bytes_per_launch"])
    # the two conv_trunk_kernel launches of the committed step trace (same box): (forward + backward) / 66 within 5 % of the line
    durs = [float(ln[64:].split()[1]) for ln in open(os.path.join(ROOT, "profiles", "r6_step_edsr_baseline_b256.txt")) if ln.startswith("conv_trunk_kernel")]
    assert len(durs) == 2
    trace_frac = 2.0 * 256 * 48 * 48 * 64 * 64 * 9 / (sum(durs) / 66 * 1e-6) / 1e12 / r["peak"]
    assert abs(trace_frac - r["frac"]) / trace_frac < 0.05, (trace_frac, r["frac"])
    for e in line["other_configs"]:
        assert "model_mfma_frac_executed" in e and "model_mfma_frac" in e, e.get("model")
        if e.get("dtype", "bf16") == "bf16" and e["model"] != "srresnet":          # (SRResNet's quoted kernel is conv_pair: measured in ITS step too)
            rr = e["roofline"]
            assert rr.get("traffic") and rr.get("algorithmic_bytes_per_launch"), e["model"]
    tn = line["cpu_baseline"]["parity"]["trained_net"]
    d = tn["delta_psnr_db"]
    assert abs(d["fp16"]) < 0.01 and abs(d["bf16_model_eval_dtype_path"]) < 0.01 and abs(d["bf16"]) < 0.03, d
    # the all-cores figure SURVEY 8(d) defines (os.cpu_count() threads) was measured once and is named in every line (it takes ~100 s on this host)
    assert "all_cores" in line["cpu_baseline"]
    first = json.loads(open(os.path.join(ROOT, "profiles", "r6_bench_default_first.json")).readline())["cpu_baseline"]
    assert first["all_cores"]["cores"] == first["cores_available"] and first["all_cores"]["value"] > 0


def test_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        return
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert not out.stdout.strip().startswith("{"), "no JSON line (no number) without the GPU"
