#!/usr/bin/env python3
"""The VGG perceptual loss (csrc/vgg_loss.hip around srk_conv2d, through sr_amd.vgg_loss) against the same loss composed from torch's own
conv / pool ops in the same storage dtype on the same GPU, in one run; and the error pairs of tests/test_gpu_vgg_loss.py.

  microbench_vgg_loss.py                  forward + backward at the training shape 16 x 3 x 192 x 192, relu2_2 and relu5_4 of vgg19 with
                                          seeded random weights: device events after warm-up, the median and the spread of --repeats timed
                                          runs of --iters steps each, and the peak allocated memory of one step above what the inputs hold;
                                          then, per (net, layer, storage dtype), the worst relative errors of the HIP path against float64
                                          next to the yardstick's (tests/vgg_ref.py) over the tests' shapes and criteria
  microbench_vgg_loss.py --kernels-only   only the HIP forward + backward (for a `rocprofv3 --kernel-trace --stats` run)
  --out FILE                              where the report goes (default profiles/vgg_loss.txt)

The eager form is what a user writes today with a torchvision-shaped stack: normalise, features of sr, features of hr under no_grad,
mse_loss, times rescale; weights and activations in the storage dtype, in torch's default (NCHW) and in channels_last memory format.
Nobody has promised a ratio: the file records what is measured, also where a shape is slower than torch's."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
RESCALE = 0.006


def images(n, size=192, seed=0):
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(n, 3, size, size, generator=g)
    sr = hr + 0.05 * torch.randn(n, 3, size, size, generator=g)
    return sr.cuda(), hr.cuda()


def eager_loss(features, dtype, channels_last):
    """The loss from torch ops, the stack's weights converted once (as the HIP path packs once)."""
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    ws = [(w.cuda().to(dtype).contiguous(memory_format=fmt), b.cuda().to(dtype)) for w, b in features.convs]
    mean = torch.tensor((0.485, 0.456, 0.406), device="cuda").view(1, 3, 1, 1)
    std = torch.tensor((0.229, 0.224, 0.225), device="cuda").view(1, 3, 1, 1)

    def f(x):
        x = ((x - mean) / std).to(dtype).contiguous(memory_format=fmt)
        it = iter(ws)
        for step in features.plan:
            if step[0] == "pool":
                x = F.max_pool2d(x, 2, 2)
            else:
                w, b = next(it)
                x = F.relu(F.conv2d(x, w, b, padding=1))
        return x

    def loss(sr, hr):
        with torch.no_grad():
            fh = f(hr)
        return RESCALE * F.mse_loss(f(sr).float(), fh.float())
    return loss


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


def error_rows(ops, precisions=tuple(DTYPES)):
    """Per (net, layer, storage dtype): the worst relative errors against float64 over the tests' shapes and both criteria, the HIP
    path's next to the yardstick's of the same case (the loss next to the largest yardstick error of that dtype and layer)."""
    import vgg_ref as REF
    for net, layer in REF.NETS_LAYERS:
        feats = ops.VGGFeatures(REF.weights(net, layer), net, layer)
        for precision in precisions:
            dtype = DTYPES[precision]
            worst = {"features": (0.0, 0.0, 0.0), "gradient": (0.0, 0.0, 0.0)}          # (ratio, hip, yardstick)
            loss_hip, loss_yard = 0.0, 0.0
            for n2, l2 in REF.NETS_LAYERS:
                if l2 == layer:
                    for shape in REF.SHAPES:
                        y = REF.yardstick(n2, l2, shape, precision)
                        loss_yard = max(loss_yard, y["l2"][0], y["l1"][0])
            for shape in REF.SHAPES:
                ref, yard = REF.reference(net, layer, shape), REF.yardstick(net, layer, shape, precision)
                sr, hr = REF.images(shape)
                ef = REF.rel(ops.vgg_features(sr.cuda(), feats, dtype).cpu(), ref["fs"])
                worst["features"] = max(worst["features"], (ef / yard["features"], ef, yard["features"]))
                for crit in REF.CRITERIA:
                    s = sr.cuda().requires_grad_(True)
                    loss = ops.VGGLossFn.apply(s, hr.cuda(), feats, REF.RESCALE, crit, dtype)
                    loss.backward()
                    eg = REF.rel(s.grad.cpu(), ref[crit][1])
                    worst["gradient"] = max(worst["gradient"], (eg / yard[crit][1], eg, yard[crit][1]))
                    loss_hip = max(loss_hip, abs(float(loss.detach()) - float(ref[crit][0])) / abs(float(ref[crit][0])))
            yield {"errors": f"{net} {layer}", "dtype": precision,
                   "features_hip_yardstick": [float(f"{v:.3e}") for v in worst["features"][1:]], "features_ratio": round(worst["features"][0], 2),
                   "gradient_hip_yardstick": [float(f"{v:.3e}") for v in worst["gradient"][1:]], "gradient_ratio": round(worst["gradient"][0], 2),
                   "loss_hip_yardstick_max": [float(f"{loss_hip:.3e}"), float(f"{loss_yard:.3e}")], "loss_ratio": round(loss_hip / loss_yard, 2)}


HEADER = """tools/microbench_vgg_loss.py on one MI355X, {date}: the VGG perceptual loss (csrc/vgg_loss.hip around srk_conv2d, through sr_amd.vgg_loss) at
16 x 3 x 192 x 192, vgg19 with seeded He-normal weights, against the same loss composed from torch's conv2d / relu / max_pool2d in the same storage dtype on
the same GPU in the same run.  us per forward + backward, launched eagerly (no graph), device events around {iters} back-to-back steps (eager forms: {eiters})
after 3 warm-up steps, median [min, max] of {repeats} such windows; peak_MiB = the most one step allocates above the two inputs and the gradient holder.
Profiler off.

  hip                 VGGLossFn: prepare, conv + bias + ReLU per layer on the frozen packs, max-pools, feature loss; backward on the SR half only
  eager_nchw          normalise, f(sr), f(hr) under no_grad, mse_loss * rescale; weights and activations in the storage dtype, NCHW
  eager_channels_last the same with weights and activations in channels_last memory format
  ratio               the FASTER eager form over hip (>= 1: the HIP path is at least as fast); no ratio was promised, this is what was measured

Then one line per (net, layer, storage dtype) of tests/test_gpu_vgg_loss.py: the worst relative error against float64 over the tests' three shapes and two
criteria, [HIP path, yardstick of that case] and their ratio (the tests allow 4); for the scalar loss the yardstick is the largest one of that dtype and layer.
Last, fp32 storage at three widths of vgg_loss.FP32_SLICE (the reduction channels per srk_conv2d launch; 512 would be one launch per conv): the relu5_4 step
and the worst fp32 ratios over all nets and layers.  A ratio in the thousands is one ReLU or max-pool decision that fell the other way, not rounding.
"""


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=16)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--no-errors", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgg_loss.txt"))
    a = p.parse_args()
    import sr_amd
    import vgg_ref as REF
    ops = sr_amd.ops
    sr, hr = images(a.n, seed=a.n)
    cases = [("relu2_2", "bf16"), ("relu2_2", "fp16"), ("relu2_2", "fp32"), ("relu5_4", "bf16"), ("relu5_4", "fp16"), ("relu5_4", "fp32")]
    eiters = max(2, a.iters // 3)
    lines = []
    # the error pairs first (seconds), written behind the timings
    errors = [] if (a.kernels_only or a.no_errors) else [json.dumps(row) for row in error_rows(ops)]

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        if not a.kernels_only:          # rewritten after every line: a run that is cut short leaves what it measured
            with open(a.out, "w") as f:
                f.write(HEADER.format(date=datetime.date.today().isoformat(), iters=a.iters, eiters=eiters, repeats=a.repeats) + "\n")
                f.write("\n".join(lines + errors) + "\n")

    for layer, precision in cases:
        dtype = DTYPES[precision]
        feats = ops.VGGFeatures(REF.weights("vgg19", layer), "vgg19", layer)
        us = time_fb(lambda s, h: ops.VGGLossFn.apply(s, h, feats, RESCALE, "l2", dtype), sr, hr, a.iters, a.repeats)
        row = {"loss": "vgg", "net": "vgg19", "layer": layer, "dtype": precision, "shape": f"{a.n}x3x192x192",
               "hip_fwd_bwd_us": round(us[0], 1), "hip_min_max_us": [round(us[1], 1), round(us[2], 1)], "hip_peak_MiB": round(us[3] / 2 ** 20, 1)}
        if not a.kernels_only:
            best = None
            for form, cl in (("nchw", False), ("channels_last", True)):
                ue = time_fb(eager_loss(feats, dtype, cl), sr, hr, eiters, a.repeats)
                row[f"eager_{form}_us"], row[f"eager_{form}_min_max_us"] = round(ue[0], 1), [round(ue[1], 1), round(ue[2], 1)]
                row[f"eager_{form}_peak_MiB"] = round(ue[3] / 2 ** 20, 1)
                best = ue[0] if best is None else min(best, ue[0])
            row["ratio_faster_eager_over_hip"] = round(best / us[0], 2)
        emit(row)
        del feats
        torch.cuda.empty_cache()
    for line in errors:
        print(line, flush=True)
    if not a.kernels_only and not a.no_errors:
        # fp32 storage cuts a conv's reduction into launches over vgg_loss.FP32_SLICE channels: what the width costs and buys
        V = sr_amd.vgg_loss
        default = V.FP32_SLICE
        for width in (16, 32, 64):
            V.FP32_SLICE = width
            feats = ops.VGGFeatures(REF.weights("vgg19", "relu5_4"), "vgg19", "relu5_4")
            us = time_fb(lambda s, h: ops.VGGLossFn.apply(s, h, feats, RESCALE, "l2", torch.float32), sr, hr, a.iters, a.repeats)
            rows = list(error_rows(ops, ("fp32",)))
            errors.append(json.dumps({"fp32_slice": width, "default": width == default, "relu5_4_hip_fwd_bwd_us": round(us[0], 1),
                                      "worst_features_ratio": max(r["features_ratio"] for r in rows),
                                      "worst_gradient_ratio": max(r["gradient_ratio"] for r in rows),
                                      "worst_loss_ratio": max(r["loss_ratio"] for r in rows)}))
            print(errors[-1], flush=True)
            del feats
        V.FP32_SLICE = default
        with open(a.out, "w") as f:
            f.write(HEADER.format(date=datetime.date.today().isoformat(), iters=a.iters, eiters=eiters, repeats=a.repeats) + "\n")
            f.write("\n".join(lines + errors) + "\n")


if __name__ == "__main__":
    main()
