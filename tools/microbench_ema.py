#!/usr/bin/env python3
"""EMA of the weights (csrc/ema.hip through sr_amd.ema.ParamEMA) against the torch forms on the same GPU, on the real parameter
sets of RCAN and EDSR-baseline (bench.py's configurations):

  update   ParamEMA.update()  (one launch)          vs  torch._foreach_lerp_(shadows, params, 1 - decay)
  swap     ParamEMA.swap()    (one launch)          vs  a per-tensor exchange in torch ops: t = p.clone(); p.copy_(s); s.copy_(t)
                                                    and its multi-tensor form (_foreach_copy_ through a list of clones)

Device events around `--iters` back-to-back calls after a warm-up, the median / min / max of `--repeats` such windows, the two sides
alternating inside every repeat.  The calls are issued launch by launch from Python (as a validation-time swap is); inside a replayed
hipGraph the host side of either form disappears and only the device time of the launches is left.  GB/s: the bytes the operation
must move (12 B per parameter for the update, 16 B for the swap) over the time of a call.  `*_replayed`: the same update captured
into a hipGraph of its own and replayed, which is how the training step runs it.  One JSON line per model."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

MODELS = {"edsr_baseline": ("EDSR", dict(n_feats=64, n_resblocks=16, res_scale=0.1)),
          "rcan": ("RCAN", dict(n_feats=64, reduction=16, n_resgroups=10, n_resblocks=20))}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def compare(fns, iters, repeats, warm=5):
    """us per call of every entry of `fns`: (median, min, max) over `repeats` windows, the entries alternating."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            runs[k].append(window(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--decay", type=float, default=0.999)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_ema.py times GPU launches: no GPU here")
    import sr_amd
    for name in a.models:
        cls, kw = MODELS[name]
        torch.manual_seed(0)
        m = getattr(sr_amd, cls)(scale_factor=4, **kw).cuda()
        ps = [q for q in m.parameters() if q.is_floating_point()]
        n = sum(q.numel() for q in ps)
        ema = sr_amd.ema.ParamEMA(ps, a.decay)
        shadows = [q.detach().clone() for q in ps]
        data = [q.detach() for q in ps]
        w = 1.0 - a.decay

        def torch_swap_each():
            for q, s in zip(data, shadows):
                t = q.clone()
                q.copy_(s)
                s.copy_(t)

        def torch_swap_foreach():
            t = [q.clone() for q in data]
            torch._foreach_copy_(data, shadows)
            torch._foreach_copy_(shadows, t)

        def captured(fn):
            g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st), torch.cuda.graph(g, stream=st):
                fn()
            torch.cuda.current_stream().wait_stream(st)
            return g

        def lerp():
            torch._foreach_lerp_(shadows, data, w)

        with torch.no_grad():
            ema.update()
            lerp()
            torch.cuda.synchronize()
            g_hip, g_torch = captured(ema.update), captured(lerp)
            r = compare({"hip_update": ema.update, "torch_foreach_lerp": lerp,
                         "hip_update_replayed": g_hip.replay, "torch_foreach_lerp_replayed": g_torch.replay,
                         "hip_swap": ema.swap, "torch_swap_per_tensor": torch_swap_each, "torch_swap_foreach": torch_swap_foreach},
                        a.iters, a.repeats)
        out = {"model": name, "tensors": len(ps), "parameters": n, "blocks": ema._table.nblocks, "iters": a.iters, "repeats": a.repeats}
        for k, (med, lo, hi) in r.items():
            out[k + "_us"] = round(med, 1)
            out[k + "_min_max_us"] = [round(lo, 1), round(hi, 1)]
        out["hip_update_GB_per_s"] = round(12 * n / (r["hip_update"][0] * 1e-6) / 1e9, 1)
        out["hip_swap_GB_per_s"] = round(16 * n / (r["hip_swap"][0] * 1e-6) / 1e9, 1)
        out["update_speedup"] = round(r["torch_foreach_lerp"][0] / r["hip_update"][0], 1)
        out["update_speedup_replayed"] = round(r["torch_foreach_lerp_replayed"][0] / r["hip_update_replayed"][0], 1)
        out["swap_speedup_vs_per_tensor"] = round(r["torch_swap_per_tensor"][0] / r["hip_swap"][0], 1)
        out["swap_speedup_vs_foreach"] = round(r["torch_swap_foreach"][0] / r["hip_swap"][0], 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
