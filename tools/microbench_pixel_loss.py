#!/usr/bin/env python3
"""The cost of the pixel losses (sr_amd.pixel_loss, csrc/pixel_loss.hip) at the HR tensor of the default bench step, 256 x 3 x 192 x 192
fp32 (28,311,552 elements, 113 MB per image tensor), next to the existing L1 launches, which are the yardstick, and to the torch
expression of the same loss (`pixel_loss_torch`, what a user would write) on the GPU.

  l1                    ops.L1LossFn: forward 9 B per element (two reads, a sign byte), backward 5 B: 14 B
  <loss>                forward + mean + backward of the HIP path: forward 8 B, backward 12 B: 20 B
  <loss>_torch_graphed  the torch expression and its autograd, captured
  <loss>_torch_eager    the same, launched eagerly

Every entry but the eager ones is forward + mean (or finalize) + backward captured into a hipGraph of its own and replayed, which is
how the training step runs it; device events around `--iters` back-to-back replays after a warm-up, median [min, max] of `--repeats`
such windows, the entries alternating inside every repeat.  One JSON line.  `expected_us` of a loss is L1's time scaled by the bytes
moved (20 / 14)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from microbench_lr_sched import captured, compare  # noqa: E402

LOSSES = {
    "charbonnier": ("charbonnier", {"eps": 1e-3}),
    "huber": ("huber", {"delta": 0.5}),
    "smooth_l1": ("smooth_l1", {"beta": 0.5}),
    "robust_a2": ("robust", {"alpha": 2.0, "c": 0.1}),
    "robust_a0": ("robust", {"alpha": 0.0, "c": 0.1}),
    "robust_neg_inf": ("robust", {"alpha": -math.inf, "c": 0.1}),
    "robust_general": ("robust", {"alpha": -2.0, "c": 0.1}),
    "psnr": ("psnr", {}),
}
L1_BYTES, HIP_BYTES = 14, 20


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", type=int, nargs=4, default=[256, 3, 192, 192])
    p.add_argument("--losses", nargs="+", default=list(LOSSES), choices=list(LOSSES))
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=7)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_pixel_loss.py times GPU launches: no GPU here")
    import sr_amd
    P = sr_amd.pixel_loss
    g = torch.Generator(device="cuda").manual_seed(0)
    hr = torch.rand(a.shape, device="cuda", generator=g)
    sr = (hr + 0.05 * torch.randn(a.shape, device="cuda", generator=g)).requires_grad_(True)

    def step(fn):
        def run():
            sr.grad = None
            fn(sr, hr).backward()
        return run

    def graphed(fn):
        run = step(fn)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                  # autograd's and the allocator's first-use work stays outside the capture
            for _ in range(3):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        return captured(run).replay

    fns = {"l1": graphed(sr_amd.ops.l1_loss)}
    for key in a.losses:
        kind, params = LOSSES[key]
        hip = getattr(P, kind + "_loss")
        fns[key] = graphed(lambda s, h, hip=hip, params=params: hip(s, h, **params))
        expr = lambda s, h, kind=kind, params=params: P.pixel_loss_torch(kind, s, h, **params)      # noqa: E731
        fns[key + "_torch_graphed"] = graphed(expr)
        fns[key + "_torch_eager"] = step(expr)
    torch.cuda.synchronize()
    r = compare(fns, a.iters, a.repeats)
    n = sr.numel()
    out = {"shape": a.shape, "elements": n, "iters": a.iters, "repeats": a.repeats, "l1_bytes_per_element": L1_BYTES,
           "hip_bytes_per_element": HIP_BYTES, "expected_us": round(r["l1"][0] * HIP_BYTES / L1_BYTES, 2)}
    for k, (med, lo, hi) in r.items():
        out[k + "_us"] = round(med, 2)
        out[k + "_min_max_us"] = [round(lo, 2), round(hi, 2)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
