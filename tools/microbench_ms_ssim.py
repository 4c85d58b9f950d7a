#!/usr/bin/env python3
"""MS-SSIM on the device (csrc/ms_ssim.hip through ops.ms_ssim) against the plain-torch fp32 path of the model (srmodel._ms_ssim_torch on
the same device tensors: pad / avg_pool2d / depthwise 11x11 conv2d per level).

  microbench_ms_ssim.py                 both paths at 1x3x1356x2040 (a DIV2K validation image), 1x3x512x512, 1x3x321x481 and
                                        16x3x192x192; device events after warm-up; the inputs fit in the Infinity Cache, so these
                                        are warm-cache times
  microbench_ms_ssim.py --kernels-only  only the HIP path at --shape (for a `rocprofv3 --kernel-trace --stats` run)
  microbench_ms_ssim.py --stats F       achieved bytes/s of the MS-SSIM kernels from that run's kernel_stats.csv (--output-format
                                        csv) or its results .db (the default rocpd output); --shape as in the run

Bytes are what the algorithm must move: both level-0 images read once, and levels 1-4 of both images written once and read once
(the pooling launch of level k reads level k-1 too).  Per kernel: ms_pool_kernel reads level k-1 and writes level k of both
images (summed over the four launches); ms_maps_kernel reads all five levels of both images once; halo re-reads are not counted."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SHAPES = [(1, 3, 1356, 2040), (1, 3, 512, 512), (1, 3, 321, 481), (16, 3, 192, 192)]


def levels(h, w):
    out = [(h, w)]
    for _ in range(4):
        p = max(h % 2, w % 2)
        h, w = (h + p) // 2, (w + p) // 2
        out.append((h, w))
    return out


def traffic(shape):
    """-> (pool bytes, maps bytes, algorithmic total) for both images."""
    n, c, h, w = shape
    px = [n * c * a * b for a, b in levels(h, w)]
    pool = sum(2 * 4 * (px[k - 1] + px[k]) for k in range(1, 5))
    maps = 2 * 4 * sum(px)
    total = 2 * 4 * px[0] + 2 * 2 * 4 * sum(px[1:])
    return pool, maps, total


def images(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(*shape, generator=g)
    sr = (hr + 0.05 * torch.randn(*shape, generator=g)).clamp(0, 1)
    return sr.cuda(), hr.cuda()


def time_call(fn, x, y, iters, warm=3):
    for _ in range(warm):
        fn(x, y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(x, y)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_stats(path, shape):
    rows = {}
    if path.endswith(".db"):
        import sqlite3
        for name, calls, avg in sqlite3.connect(path).execute("select name, total_calls, average from top_kernels"):
            if "ms_" in name:
                rows[name] = (float(avg) * 1e3, int(calls))         # average in us
    else:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                if "ms_" in name:
                    rows[name] = (float(r["AverageNs"]), int(r["Calls"]))
    pool, maps, total = traffic(shape)
    res = {}
    for name, (ns, calls) in rows.items():
        b = maps if "maps" in name else None
        res[name] = {"avg_us": ns / 1e3, "calls": calls, "GB_per_s": (b / (ns * 1e-9) / 1e9) if b else None}
    pool_ns = sum(ns * calls for name, (ns, calls) in rows.items() if "pool" in name)
    maps_calls = sum(calls for name, (ns, calls) in rows.items() if "maps" in name)
    if pool_ns and maps_calls:
        res["ms_pool_kernel (4 levels, per call)"] = {"us": pool_ns / maps_calls / 1e3, "GB_per_s": pool / (pool_ns / maps_calls * 1e-9) / 1e9}
    all_ns = sum(ns * calls for ns, calls in rows.values())
    if all_ns and maps_calls:
        res["all kernels, per call"] = {"us": all_ns / maps_calls / 1e3, "algorithmic_GB_per_s": total / (all_ns / maps_calls * 1e-9) / 1e9}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--shape", default="1x3x1356x2040")
    p.add_argument("--stats", default=None)
    a = p.parse_args()
    shape = tuple(int(v) for v in a.shape.split("x"))
    if a.stats is not None:
        print(json.dumps({"shape": a.shape, "kernels": kernel_stats(a.stats, shape)}))
        return
    import sr_amd
    from sr_amd.models.srmodel import _ms_ssim_torch as torch_path
    ops = sr_amd.ops
    if a.kernels_only:
        x, y = images(shape)
        us = time_call(ops.ms_ssim, x, y, a.iters)
        print(json.dumps({"shape": a.shape, "hip_us": round(us, 1)}))
        return
    res = {}
    for shape in SHAPES:
        x, y = images(shape, seed=sum(shape))
        hip = time_call(ops.ms_ssim, x, y, a.iters)
        tor = time_call(torch_path, x, y, max(3, a.iters // 4))
        d = abs(float(ops.ms_ssim(x, y)) - float(torch_path(x, y)))
        key = "x".join(map(str, shape))
        res[key] = {"hip_us": round(hip, 1), "torch_us": round(tor, 1), "speedup": round(tor / hip, 1), "abs_diff": d,
                    "algorithmic_MB": round(traffic(shape)[2] / 1e6, 1)}
        print(json.dumps({key: res[key]}), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
