#!/usr/bin/env python3
"""MS-SSIM loss (csrc/ms_ssim_loss.hip through sr_amd.ms_ssim_loss) against the eager torch form
(1 - ms_ssim_torch(clamp(sr), hr)) on the same GPU.

  microbench_ms_ssim_loss.py                 HIP forward + backward vs the eager torch forward + backward at 16 and 256 x 3 x 192 x 192
                                             (device events after warm-up; the median of --repeats timed runs of --iters iterations)
  microbench_ms_ssim_loss.py --kernels-only  only the HIP forward + backward at --n (for a `rocprofv3 --kernel-trace --stats` run)

Bytes the algorithm must move per pixel of a plane, for the GB/s figure: the five levels hold 1 + 1/4 + ... + 1/256 = 1.332 pixels.
Forward: read sr and hr (8 B), write and read back levels 1-4 of both (0.332 x 16 B).  Backward: read both images of every level
(1.332 x 8 B), write and read back the gradients of levels 1-4 (0.332 x 8 B), write grad (4 B).  Halo re-reads and the per-tile sums
are not counted."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

BYTES_PER_PIXEL = (8 + 0.332 * 16) + (1.332 * 8 + 0.332 * 8 + 4)


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=16)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernels-only", action="store_true")
    a = p.parse_args()
    import sr_amd
    ops = sr_amd.ops
    if a.kernels_only:
        sr, hr = images(a.n)
        us = time_fb(ops.MSSSIMLossFn.apply, sr, hr, a.iters, a.repeats)
        print(json.dumps({"n": a.n, "hip_fwd_bwd_us": round(us[0], 1), "min_us": round(us[1], 1), "max_us": round(us[2], 1)}))
        return
    for n in (16, 256):
        sr, hr = images(n, seed=n)
        hip = time_fb(ops.MSSSIMLossFn.apply, sr, hr, a.iters, a.repeats)
        eager = time_fb(lambda s, h: 1.0 - ops.ms_ssim_torch(s.clamp(0, 1), h), sr, hr, max(3, a.iters // 4), a.repeats)
        pix = n * 3 * 192 * 192
        res = {"hip_fwd_bwd_us": round(hip[0], 1), "hip_min_max_us": [round(hip[1], 1), round(hip[2], 1)],
               "torch_eager_fwd_bwd_us": round(eager[0], 1), "torch_min_max_us": [round(eager[1], 1), round(eager[2], 1)],
               "speedup": round(eager[0] / hip[0], 1), "hip_GB_per_s": round(BYTES_PER_PIXEL * pix / (hip[0] * 1e-6) / 1e9, 1)}
        print(json.dumps({f"{n}x3x192x192": res}), flush=True)


if __name__ == "__main__":
    main()
