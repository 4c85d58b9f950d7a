#!/usr/bin/env python3
"""The HIP SGD and RMSprop steps (csrc/optim.hip `srk_sgd_step`, `srk_rmsprop_step`) against the HIP Adam step and against
`torch.optim.SGD` / `torch.optim.RMSprop`, over the parameter sets of RCAN and EDSR-baseline (x4, the reference's default
configurations).

HIP variants: SGD plain (p read + written, g read = 12 B per parameter) and with momentum (20 B); RMSprop plain (20 B) and
with momentum and centering (36 B); Adam (28 B).  The torch variants are built as `configure_optimizers()` built them before
the HIP classes existed: `torch.optim.SGD(params)` / `torch.optim.RMSprop(params)` at torch's defaults (foreach on the GPU).

Each step is captured into a hipGraph and replayed (no Python between steps) where it captures; a torch step that refuses
the capture is timed launch by launch instead, and the output says which ("replayed" / "eager").  Device events around
`--iters` steps after `--warm` give the time per step.  The variants alternate within each of `--rounds` rounds; the median and
the spread over rounds are printed, then one JSON line.

  microbench_optim.py [--iters 200] [--warm 20] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

# variant -> (bytes per parameter of the HIP kernel or None, the torch variant it is held against or None)
VARIANTS = {
    "sgd": (12, "torch_sgd"),
    "sgd_momentum": (20, "torch_sgd"),
    "rmsprop": (20, "torch_rmsprop"),
    "rmsprop_momentum_centered": (36, "torch_rmsprop"),
    "adam": (28, None),
    "torch_sgd": (None, None),
    "torch_rmsprop": (None, None),
}


def param_shapes(name):
    import sr_amd
    m = sr_amd.RCAN(scale_factor=4) if name == "RCAN" else sr_amd.EDSR(scale_factor=4, n_feats=64, n_resblocks=16)
    return [tuple(p.shape) for p in m.parameters() if p.requires_grad]


def make(kind, ps):
    import sr_amd
    O = sr_amd.optim
    return {"sgd": lambda: O.SGD(ps), "sgd_momentum": lambda: O.SGD(ps, momentum=0.9),
            "rmsprop": lambda: O.RMSprop(ps), "rmsprop_momentum_centered": lambda: O.RMSprop(ps, momentum=0.9, centered=True),
            "adam": lambda: O.Adam(ps), "torch_sgd": lambda: torch.optim.SGD(ps), "torch_rmsprop": lambda: torch.optim.RMSprop(ps)}[kind]()


def prepared_step(kind, shapes, seed=0):
    """(callable that runs one step, "replayed" or "eager", what must stay alive)."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(((torch.rand(*s, generator=g) - 0.5) * 0.1).cuda()) for s in shapes]
    for p in ps:
        p.grad = ((torch.rand(*p.shape, generator=g) - 0.5) * 1e-2).cuda()
    opt = make(kind, ps)
    for _ in range(2):
        opt.step()
    torch.cuda.synchronize()
    if opt.defaults.get("capturable") is False and kind.startswith("torch_"):
        # torch's step raises inside a capture unless it was built capturable (RMSprop; configure_optimizers() never did)
        return opt.step, "eager", (ps, opt)
    if hasattr(opt, "reserve_capture_tables"):
        opt.reserve_capture_tables()
    graph = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(st):
            with torch.cuda.graph(graph, stream=st):
                opt.step()
    except Exception as e:                                   # a torch step that refuses the capture for another reason
        if not kind.startswith("torch_"):
            raise
        print(f"{kind}: not capturable ({str(e).splitlines()[0][:100]}): timed launch by launch", flush=True)
        torch.cuda.synchronize()
        return opt.step, "eager", (ps, opt)
    torch.cuda.current_stream().wait_stream(st)
    return graph.replay, "replayed", (ps, opt, graph)


def time_steps(step, iters, warm):
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
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
        raise SystemExit("microbench_optim.py needs a GPU")
    result = {}
    for model in ("RCAN", "EDSR-baseline"):
        shapes = param_shapes(model)
        n = sum(torch.Size(s).numel() for s in shapes)
        steps = {kind: prepared_step(kind, shapes) for kind in VARIANTS}
        times = {kind: [] for kind in VARIANTS}
        for _ in range(a.rounds):
            for kind, (step, _, _) in steps.items():
                times[kind].append(time_steps(step, a.iters, a.warm))
        row = {"params": n, "tensors": len(shapes)}
        for kind, ts in times.items():
            med, nbytes = statistics.median(ts), VARIANTS[kind][0]
            row[kind] = {"us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2), "mode": steps[kind][1]}
            line = f"{model:14s} {kind:26s} {steps[kind][1]:8s} {n / 1e6:7.2f} M params  {med:9.1f} us  (min {min(ts):.1f}, max {max(ts):.1f})"
            if nbytes:
                row[kind]["GBps"] = round(nbytes * n / med / 1e3, 1)
                line += f"  {nbytes * n / med / 1e3:7.1f} GB/s at {nbytes} B/param"
            print(line, flush=True)
        for kind, (_, against) in VARIANTS.items():
            if against:
                row[kind]["over_" + against] = round(row[kind]["us"] / row[against]["us"], 4)
            if kind != "adam" and not kind.startswith("torch_"):
                row[kind]["over_adam"] = round(row[kind]["us"] / row["adam"]["us"], 3)
        result[model] = row
        del steps
        torch.cuda.synchronize()
    print(json.dumps({"microbench": "sgd_rmsprop_vs_torch", "iters": a.iters, "rounds": a.rounds, "result": result}))


if __name__ == "__main__":
    main()
