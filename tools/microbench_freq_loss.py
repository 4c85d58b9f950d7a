#!/usr/bin/env python3
"""Frequency losses (csrc/freq_loss.hip through sr_amd.freq_loss) against the eager torch.fft forms on the same GPU, in one run.

  microbench_freq_loss.py                 forward + backward of the HIP path and of the eager expressions at 16 and 256 x 3 x 192 x 192:
                                          device events after warm-up, the median and the spread of --repeats timed runs of --iters
                                          steps each, and the peak allocated memory of one step above what the inputs hold
  microbench_freq_loss.py --kernels-only  only the HIP forward + backward at --n (for a `rocprofv3 --kernel-trace --stats` run)

The eager forms are what a user writes today:
  fft (BasicSR)   l1_loss(stack(fft2(sr).real, fft2(sr).imag), stack(fft2(hr).real, fft2(hr).imag)): BasicSR's FFTLoss.forward
  fft (one fft2)  the same value from ONE transform, stack(fft2(sr - hr).real, .imag).abs().mean(): the cheaper eager form
  ffl             FocalFrequencyLoss with patch_factor=1: fft2(norm="ortho") of both images, the weight matrix under no_grad
The bar for the HIP path is the faster eager form of each loss."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def images(n, size=192, seed=0):
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(n, 3, size, size, generator=g)
    sr = hr + 0.05 * torch.randn(n, 3, size, size, generator=g)
    return sr.cuda(), hr.cuda()


def eager_fft_basicsr(sr, hr):
    a, b = torch.fft.fft2(sr, dim=(-2, -1)), torch.fft.fft2(hr, dim=(-2, -1))
    return F.l1_loss(torch.stack([a.real, a.imag], dim=-1), torch.stack([b.real, b.imag], dim=-1))


def eager_fft_one(sr, hr):
    d = torch.fft.fft2(sr - hr, dim=(-2, -1))
    return torch.stack([d.real, d.imag], dim=-1).abs().mean()


def eager_ffl(sr, hr, alpha=1.0):
    a, b = torch.fft.fft2(sr, norm="ortho"), torch.fft.fft2(hr, norm="ortho")
    q = (a.real - b.real) ** 2 + (a.imag - b.imag) ** 2
    with torch.no_grad():
        w = torch.sqrt(q) ** alpha
        w = w / w.amax(dim=(-2, -1), keepdim=True)
        w = torch.nan_to_num(w, nan=0.0).clamp(0.0, 1.0)
    return (w * q).mean()


def time_fb(fn, sr, hr, iters, repeats, warm=3):
    """(median, min, max) us of forward + backward, and the peak bytes one step allocates above the inputs."""
    s = sr.detach().clone().requires_grad_(True)

    def once():
        s.grad = None
        fn(s, hr).backward()
    for _ in range(warm):
        once()
    torch.cuda.synchronize()
    s.grad = None
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    once()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            once()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(runs), min(runs), max(runs), peak


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=16)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--kernels-only", action="store_true")
    a = p.parse_args()
    import sr_amd
    ops = sr_amd.ops
    hip = {"fft": ops.FFTLossFn.apply, "ffl": lambda s, h: ops.FFLLossFn.apply(s, h, 1.0)}
    if a.kernels_only:
        sr, hr = images(a.n)
        for name, fn in hip.items():
            us = time_fb(fn, sr, hr, a.iters, a.repeats)
            print(json.dumps({"loss": name, "n": a.n, "hip_fwd_bwd_us": round(us[0], 1), "min_us": round(us[1], 1), "max_us": round(us[2], 1)}))
        return
    eager = {"fft": {"basicsr": eager_fft_basicsr, "one_fft2": eager_fft_one}, "ffl": {"ffl": eager_ffl}}
    for n in (16, 256):
        sr, hr = images(n, seed=n)
        for name, fn in hip.items():
            row = {}
            us = time_fb(fn, sr, hr, a.iters, a.repeats)
            row["hip_fwd_bwd_us"], row["hip_min_max_us"], row["hip_peak_MiB"] = round(us[0], 1), [round(us[1], 1), round(us[2], 1)], round(us[3] / 2 ** 20, 1)
            best = None
            for form, efn in eager[name].items():
                ue = time_fb(efn, sr, hr, max(3, a.iters // 4), a.repeats)
                row[f"eager_{form}_us"], row[f"eager_{form}_min_max_us"] = round(ue[0], 1), [round(ue[1], 1), round(ue[2], 1)]
                row[f"eager_{form}_peak_MiB"] = round(ue[3] / 2 ** 20, 1)
                best = ue[0] if best is None else min(best, ue[0])
            row["ratio_fastest_eager_over_hip"] = round(best / us[0], 2)
            print(json.dumps({"loss": name, "shape": f"{n}x3x192x192", **row}), flush=True)


if __name__ == "__main__":
    main()
