#!/usr/bin/env python3
"""HaarPSI loss (csrc/haarpsi.hip through sr_amd.haarpsi) against the eager torch form (1 - haarpsi_torch(clamp(sr), hr)), and its
cost in a training step.

  microbench_haarpsi.py                 HIP forward + backward vs the eager torch forward + backward at 16 and 256 x 3 x 192 x 192
                                        (device events after warm-up), then the EDSR-baseline x4 batch-16 training step
                                        (Trainer.fit, graphed) with losses="l1" and losses="0.9*l1+0.1*haarpsi", alternating
  microbench_haarpsi.py --kernels-only  only the HIP forward + backward at --n (for a `rocprofv3 --kernel-trace --stats` run)
  microbench_haarpsi.py --stats F       achieved bytes/s of the HaarPSI kernels from that run's kernel_stats.csv (--output-format
                                        csv) or its results .db (the default rocpd output); --n as in the run

Bytes are what the algorithm must move per HR pixel: forward reads sr and hr (24 B) and keeps the subsampled Y', I', Q' planes of
both images (24 B per half-res pixel: 6 B); backward reads those planes (6 B) and sr (12 B, for the clamp mask) and writes the
gradient (12 B).  Halo re-reads and the per-tile / per-image sums are not counted."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

BYTES_FWD, BYTES_BWD = 24 + 6, 6 + 12 + 12


def images(n, size=192, seed=0):
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(n, 3, size, size, generator=g)
    sr = hr + 0.05 * torch.randn(n, 3, size, size, generator=g)
    return sr.cuda(), hr.cuda()


def time_fb(fn, sr, hr, iters, warm=3):
    s = sr.detach().clone().requires_grad_(True)

    def once():
        s.grad = None
        fn(s, hr).backward()
    for _ in range(warm):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def step_times(rounds, steps, warm):
    import sr_amd
    from sr_amd import trainer as T
    out = {"l1": [], "0.9*l1+0.1*haarpsi": []}
    batches = [T.synthetic_batch(16, 3, 48, 4, 1000 + i, "cuda") for i in range(4)]
    for _ in range(rounds):
        for losses in out:
            torch.manual_seed(0)
            m = sr_amd.EDSR(scale_factor=4, precision="bf16", n_feats=64, n_resblocks=16, res_scale=0.1, losses=losses)
            ev = []

            def gen():
                for i in range(warm + steps + 1):
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    ev.append(e)
                    yield batches[i % len(batches)]
            tr = T.Trainer(device="cuda")
            tr.fit(m, gen())
            torch.cuda.synchronize()
            assert tr.graphed is not None and tr.graphed.graphs is not None and not tr.graphed.failed
            out[losses].append(ev[warm].elapsed_time(ev[warm + steps]) * 1e3 / steps)
    return out


def kernel_stats(path, n):
    pix = n * 192 * 192
    rows = {}
    if path.endswith(".db"):
        import sqlite3
        for name, calls, avg in sqlite3.connect(path).execute("select name, total_calls, average from top_kernels"):
            if "haarpsi" in name:
                rows[name] = (float(avg) * 1e3, int(calls))         # average in us
    else:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                if "haarpsi" in name:
                    rows[name] = (float(r["AverageNs"]), int(r["Calls"]))
    res = {}
    for name, (ns, calls) in rows.items():
        b = BYTES_FWD if "fwd" in name else BYTES_BWD if "bwd" in name else 0
        res[name] = {"avg_us": ns / 1e3, "calls": calls, "GB_per_s": (b * pix / (ns * 1e-9) / 1e9) if b else None}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=16)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--stats", default=None)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--steps", type=int, default=30)
    a = p.parse_args()
    if a.stats is not None:
        print(json.dumps({"n": a.n, "kernels": kernel_stats(a.stats, a.n)}))
        return
    import sr_amd
    ops = sr_amd.ops
    if a.kernels_only:
        sr, hr = images(a.n)
        us = time_fb(ops.HaarPSILossFn.apply, sr, hr, a.iters)
        print(json.dumps({"n": a.n, "hip_fwd_bwd_us": us}))
        return
    res = {}
    for n in (16, 256):
        sr, hr = images(n, seed=n)
        hip = time_fb(ops.HaarPSILossFn.apply, sr, hr, a.iters)
        eager = time_fb(lambda s, h: 1.0 - ops.haarpsi_torch(s.clamp(0, 1), h), sr, hr, max(3, a.iters // 4))
        res[f"{n}x3x192x192"] = {"hip_fwd_bwd_us": round(hip, 1), "torch_eager_fwd_bwd_us": round(eager, 1), "speedup": round(eager / hip, 1)}
        print(json.dumps({f"{n}x3x192x192": res[f"{n}x3x192x192"]}), flush=True)
    st = step_times(a.rounds, a.steps, 8)
    l1, hp = min(st["l1"]), min(st["0.9*l1+0.1*haarpsi"])
    res["edsr_baseline_x4_b16_step_us"] = {"l1": [round(v, 1) for v in st["l1"]],
                                           "0.9*l1+0.1*haarpsi": [round(v, 1) for v in st["0.9*l1+0.1*haarpsi"]],
                                           "added_pct_best": round(100.0 * (hp - l1) / l1, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
