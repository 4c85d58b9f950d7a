#!/usr/bin/env python3
"""The cost of a learning rate that is read on the device (sr_amd.lr_sched.DeviceLRSchedule; `lr_dev` of csrc/optim.hip,
csrc/lr_sched.hip), over EDSR-baseline's parameter set (bench.py's default model):

  <optimizer>_by_value      the optimizer's step, `lr` in the launch arguments           (what every step without a schedule runs)
  <optimizer>_device_lr     the same step with `lr_dev` set: one scalar load per workgroup; the schedule's own launch NOT included
  lr_sched_advance          `srk_lr_sched_step(SRK_LR_ADVANCE)` alone, one workgroup of one wave

Every entry is captured into a hipGraph of its own and replayed, which is how the training step runs it; device events around
`--iters` back-to-back replays after a warm-up, median [min, max] of `--repeats` such windows, the entries alternating inside every
repeat.  The two forms of one optimizer are two optimizer objects over two copies of the parameters with the same gradients.  One JSON
line per optimizer and one for the schedule launch."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

OPTIMIZERS = {"adam": ("Adam", {}), "ranger": ("Ranger", {}), "sgd": ("SGD", {}), "sgd_momentum": ("SGD", dict(momentum=0.9)),
              "rmsprop": ("RMSprop", {}), "rmsprop_centered_momentum": ("RMSprop", dict(centered=True, momentum=0.9))}


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


def captured(fn, prepare=None):
    if prepare is not None:
        prepare()
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st), torch.cuda.graph(g, stream=st):
        fn()
    torch.cuda.current_stream().wait_stream(st)
    return g


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--optimizers", nargs="+", default=list(OPTIMIZERS), choices=list(OPTIMIZERS))
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=7)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_lr_sched.py times GPU launches: no GPU here")
    import sr_amd
    torch.manual_seed(0)
    model = sr_amd.EDSR(scale_factor=4, n_feats=64, n_resblocks=16, res_scale=0.1).cuda()
    shapes = [q.shape for q in model.parameters() if q.requires_grad]
    n = sum(s.numel() for s in shapes)
    grads = [torch.randn(s, device="cuda") * 1e-3 for s in shapes]

    def build(name, kw, scheduled):
        ps = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.05) for s in shapes]
        for q, g in zip(ps, grads):
            q.grad = g
        opt = getattr(sr_amd.optim, name)(ps, lr=1e-4, **kw)
        sched = None
        if scheduled:
            sched = sr_amd.lr_sched.DeviceLRSchedule(opt, "cosine", t_max=300000, eta_min=1e-7)
            for h in sched._handles:         # the optimizer's launches alone: the advance is timed on its own below
                h.remove()
        opt.step()                           # the plan, outside the capture
        return opt, sched

    last = None
    for key in a.optimizers:
        name, kw = OPTIMIZERS[key]
        (ov, _), (od, sched) = build(name, kw, False), build(name, kw, True)
        last = sched
        gv, gd = captured(ov.step, ov.reserve_capture_tables), captured(od.step, od.reserve_capture_tables)
        r = compare({"by_value": gv.replay, "device_lr": gd.replay}, a.iters, a.repeats)
        out = {"optimizer": key, "tensors": len(shapes), "parameters": n, "iters": a.iters, "repeats": a.repeats}
        for k, (med, lo, hi) in r.items():
            out[k + "_us"] = round(med, 2)
            out[k + "_min_max_us"] = [round(lo, 2), round(hi, 2)]
        out["device_lr_minus_by_value_us"] = round(r["device_lr"][0] - r["by_value"][0], 2)
        print(json.dumps(out), flush=True)
        del gv, gd
        ov.release_captured_tables()
        od.release_captured_tables()
    if last is not None:
        g = captured(last.step)
        (med, lo, hi), = compare({"advance": g.replay}, a.iters, a.repeats).values()
        print(json.dumps({"launch": "lr_sched_advance", "kind": last.kind, "groups": len(last.base_lrs), "iters": a.iters, "repeats": a.repeats,
                          "advance_us": round(med, 2), "advance_min_max_us": [round(lo, 2), round(hi, 2)]}), flush=True)


if __name__ == "__main__":
    main()
