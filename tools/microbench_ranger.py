#!/usr/bin/env python3
"""The HIP Ranger step (csrc/optim.hip `srk_ranger_step`) against the HIP Adam step (`srk_adam_step`) over the parameter sets of
RCAN and EDSR-baseline (x4, the reference's default configurations).

Each optimizer's step is captured into a hipGraph and replayed (no Python between steps); device events around `--iters`
replays after `--warm` give the time per step.  Ranger is timed twice: with k = 2^30 (every step ordinary: p, m, v read and
written, g read = 28 B per parameter, Adam's traffic) and with k = 1 (every step a Lookahead sync: the slow buffer too, 36 B).
The variants alternate within each of `--rounds` rounds; the median and the spread over rounds are printed, then one JSON line.

  microbench_ranger.py [--iters 200] [--warm 20] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

BYTES = {"adam": 28, "ranger": 28, "ranger_sync": 36}


def param_shapes(name):
    import sr_amd
    m = sr_amd.RCAN(scale_factor=4) if name == "RCAN" else sr_amd.EDSR(scale_factor=4, n_feats=64, n_resblocks=16)
    return [tuple(p.shape) for p in m.parameters() if p.requires_grad]


def graphed_step(kind, shapes, seed=0):
    import sr_amd
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(((torch.rand(*s, generator=g) - 0.5) * 0.1).cuda()) for s in shapes]
    for p in ps:
        p.grad = ((torch.rand(*p.shape, generator=g) - 0.5) * 1e-2).cuda()
    opt = {"adam": lambda: sr_amd.optim.Adam(ps), "ranger": lambda: sr_amd.optim.Ranger(ps, k=1 << 30),
           "ranger_sync": lambda: sr_amd.optim.Ranger(ps, k=1)}[kind]()
    for _ in range(2):
        opt.step()
    opt.reserve_capture_tables()
    graph = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            opt.step()
    torch.cuda.current_stream().wait_stream(st)
    return graph, (ps, opt)


def time_replays(graph, iters, warm):
    for _ in range(warm):
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters             # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_ranger.py needs a GPU")
    result = {}
    for model in ("RCAN", "EDSR-baseline"):
        shapes = param_shapes(model)
        n = sum(torch.Size(s).numel() for s in shapes)
        steps = {kind: graphed_step(kind, shapes) for kind in BYTES}
        times = {kind: [] for kind in BYTES}
        for _ in range(a.rounds):
            for kind, (graph, _) in steps.items():
                times[kind].append(time_replays(graph, a.iters, a.warm))
        row = {"params": n, "tensors": len(shapes)}
        for kind, ts in times.items():
            med = statistics.median(ts)
            row[kind] = {"us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
                         "GBps": round(BYTES[kind] * n / med / 1e3, 1)}
            print(f"{model:14s} {kind:12s} {n / 1e6:7.2f} M params  {med:8.1f} us  (min {min(ts):.1f}, max {max(ts):.1f})  "
                  f"{BYTES[kind] * n / med / 1e3:7.1f} GB/s at {BYTES[kind]} B/param", flush=True)
        row["ranger_over_adam"] = round(row["ranger"]["us"] / row["adam"]["us"], 3)
        row["ranger_sync_over_adam"] = round(row["ranger_sync"]["us"] / row["adam"]["us"], 3)
        result[model] = row
        del steps
        torch.cuda.synchronize()
    print(json.dumps({"microbench": "ranger_vs_adam", "iters": a.iters, "rounds": a.rounds, "result": result}))


if __name__ == "__main__":
    main()
