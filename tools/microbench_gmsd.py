#!/usr/bin/env python3
"""GMSD loss (csrc/gmsd.hip through sr_amd.gmsd) against the eager torch form (gmsd_torch(clamp(sr), hr) with autograd) on the
same GPU.

  microbench_gmsd.py                 HIP forward + backward vs the eager torch forward + backward at 16 and 256 x 3 x 192 x 192
                                          (device events after warm-up; the median of --repeats timed runs)
  microbench_gmsd.py --kernels-only  only the HIP forward + backward at --n (for a `rocprofv3 --kernel-trace --stats` run)
  microbench_gmsd.py --stats F       achieved bytes/s of the GMSD kernels      from that run's kernel_stats.csv
                                          (--output-format csv) or its results .db (the default rocpd output); --n as in the run

Bytes are what the algorithm must move per pixel of a plane: forward reads sr and hr (8 B); backward reads sr and hr (8 B) and
writes the gradient (4 B).  Halo re-reads, the mask re-read and the per-tile sums are not counted."""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

BYTES_FWD, BYTES_BWD = 8, 8 + 4


def images(n, size=192, seed=0):
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(n, 3, size, size, generator=g)
    sr = hr + 0.05 * torch.randn(n, 3, size, size, generator=g)
    return sr.cuda(), hr.cuda()


def time_fb(fn, sr, hr, iters, repeats, warm=3):
    s = sr.detach().clone().requires_grad_(True)

    def once():
        s.grad = None
        fn(s, hr).backward()
    for _ in range(warm):
        once()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            once()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(runs), min(runs), max(runs)


def kernel_stats(path, n):
    pix = n * 3 * 192 * 192
    rows = {}
    if path.endswith(".db"):
        import sqlite3
        for name, calls, avg in sqlite3.connect(path).execute("select name, total_calls, average from top_kernels"):
            if "gmsd" in name:
                rows[name] = (float(avg) * 1e3, int(calls))         # average in us
    else:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                if "gmsd" in name:
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
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--stats", default=None)
    a = p.parse_args()
    if a.stats is not None:
        print(json.dumps({"n": a.n, "kernels": kernel_stats(a.stats, a.n)}))
        return
    import sr_amd
    ops = sr_amd.ops
    if a.kernels_only:
        sr, hr = images(a.n)
        us = time_fb(ops.GMSDLossFn.apply, sr, hr, a.iters, a.repeats)
        print(json.dumps({"n": a.n, "hip_fwd_bwd_us": round(us[0], 1), "min_us": round(us[1], 1), "max_us": round(us[2], 1)}))
        return
    res = {}
    for n in (16, 256):
        sr, hr = images(n, seed=n)
        hip = time_fb(ops.GMSDLossFn.apply, sr, hr, a.iters, a.repeats)
        eager = time_fb(lambda s, h: ops.gmsd_torch(s.clamp(0, 1), h), sr, hr, max(3, a.iters // 4), a.repeats)
        res[f"{n}x3x192x192"] = {"hip_fwd_bwd_us": round(hip[0], 1), "hip_min_max_us": [round(hip[1], 1), round(hip[2], 1)],
                                 "torch_eager_fwd_bwd_us": round(eager[0], 1), "torch_min_max_us": [round(eager[1], 1), round(eager[2], 1)],
                                 "speedup": round(eager[0] / hip[0], 1)}
        print(json.dumps({f"{n}x3x192x192": res[f"{n}x3x192x192"]}), flush=True)


if __name__ == "__main__":
    main()
