#!/usr/bin/env python3
"""The cost of gradient accumulation inside the step (sr_amd.grad_accum.GradAccum, csrc/grad_accum.hip) over the parameter tables of
EDSR-baseline (bench.py's default model) and EDSR-large, next to the EMA update over the same table (tools/microbench_ema.py's
`hip_update_replayed`, 12 B per parameter through the same walk), which is the yardstick.

  ema_update         srk_ema_step(UPDATE)                                        12 B per parameter
  accum_add          srk_grad_accum(SRK_ACCUM_ADD):   acc = acc + g                12 B
  accum_final        srk_grad_accum(SRK_ACCUM_FINAL): g = (acc + g) * inv_k; acc = 0   16 B   (inv_k = 1 here, so that replays on the same
                     gradients leave them as they are)

Every entry is captured into a hipGraph of its own (one node, an accumulator buffer of its own) and replayed, which is how the training
step runs it; device events around `--iters` back-to-back replays after a warm-up, median [min, max] of `--repeats` such windows, the
entries alternating inside every repeat.  One JSON line per model.  (Both parameter sets fit the 256 MiB Infinity Cache between
iterations: the times are not HBM rates.)

Then one line for a small training step (EDSR n_feats 32, 2 blocks, x2, 4 patches of 16x16, bf16, k = 2) captured by
`trainer.GraphedStep`: the replay time of its accumulate-phase graph and of its step-phase graph."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from microbench_grad_clip import MODELS  # noqa: E402
from microbench_lr_sched import captured, compare  # noqa: E402


def step_graphs(sr_amd, iters, repeats):
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = sr_amd.EDSR(scale_factor=2, precision="bf16", n_feats=32, n_resblocks=2, res_scale=0.1, accumulate_grad_batches=2).cuda()
    opt = m.configure_optimizers()[0]
    gs = T.GraphedStep(m, m, opt, None, warm_steps=2)
    for i in range(6):
        gs(T.synthetic_batch(4, 3, 16, 2, 900 + i, "cuda"))
    torch.cuda.synchronize()
    assert not gs.failed and set(gs.by_phase) == {"accumulate", "step"}, (gs.failed, list(gs.by_phase))
    r = compare({ph + "_graph": gs.by_phase[ph][0][0].replay for ph in ("accumulate", "step")}, iters, repeats)
    out = {"model": "edsr_small_step", "batch": 4, "k": 2, "iters": iters, "repeats": repeats}
    for k, (med, lo, hi) in r.items():
        out[k + "_us"] = round(med, 2)
        out[k + "_min_max_us"] = [round(lo, 2), round(hi, 2)]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--no-step", action="store_true", help="skip the small training step's two graphs")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_grad_accum.py times GPU launches: no GPU here")
    import sr_amd
    L = sr_amd._lib
    for key in a.models:
        torch.manual_seed(0)
        model = sr_amd.EDSR(scale_factor=4, **MODELS[key])
        shapes = [q.shape for q in model.parameters() if q.requires_grad]
        del model
        ps = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.05) for s in shapes]
        for q in ps:
            q.grad = torch.randn_like(q) * 1e-3
        opt = sr_amd.optim.SGD(ps, lr=1e-4)
        opt.step()                               # the plan and the eager table, outside any capture
        torch.cuda.synchronize()
        plan = opt._plans[0]
        t = plan.eager
        ema = sr_amd.ema.ParamEMA(ps, 0.999)
        ema.update()
        keep = []

        def entry(op):
            """One srk_grad_accum launch over the optimizer's table with an accumulator of its OWN (the entries alternate: none reads
            what another one wrote), as a function to capture."""
            acc = torch.zeros(plan.size, dtype=torch.float32, device="cuda")
            args = L.GradAccumArgs(**t.pointers(), acc=acc.data_ptr(), inv_k=1.0, op=op)
            keep.append((acc, args))
            return lambda: L.call("srk_grad_accum", args, torch.cuda.current_stream().cuda_stream)
        graphs = {
            "ema_update": captured(ema.update),
            "accum_add": captured(entry(L.SRK_ACCUM_ADD)),
            "accum_final": captured(entry(L.SRK_ACCUM_FINAL)),
        }
        torch.cuda.synchronize()
        r = compare({k: g.replay for k, g in graphs.items()}, a.iters, a.repeats)
        n = sum(s.numel() for s in shapes)
        out = {"model": key, "tensors": len(shapes), "parameters": n, "blocks": t.nblocks, "iters": a.iters, "repeats": a.repeats}
        for k, (med, lo, hi) in r.items():
            out[k + "_us"] = round(med, 2)
            out[k + "_min_max_us"] = [round(lo, 2), round(hi, 2)]
        out["add_over_ema"] = round(r["accum_add"][0] / r["ema_update"][0], 3)
        out["final_over_ema"] = round(r["accum_final"][0] / r["ema_update"][0], 3)
        print(json.dumps(out), flush=True)
        del graphs, keep, ps, opt, ema
        torch.cuda.empty_cache()
    if not a.no_step:
        print(json.dumps(step_graphs(sr_amd, a.iters, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
