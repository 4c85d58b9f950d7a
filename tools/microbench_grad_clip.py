#!/usr/bin/env python3
"""The cost of gradient clipping inside the step (sr_amd.grad_clip.GradClip, csrc/grad_clip.hip) over the parameter tables of
EDSR-baseline (bench.py's default model) and EDSR-large, next to the EMA update over the same table (tools/microbench_ema.py's
`hip_update_replayed`, 12 B per parameter), which is the yardstick: `sumsq` moves 4 B per parameter and `apply` 8 B, so neither may
take longer than it.

  ema_update         srk_ema_step(UPDATE)                                       12 B per parameter
  sumsq              srk_grad_sumsq alone                                        4 B
  coef               srk_grad_clip_coef alone (one workgroup over the partials)
  apply_clipping     srk_grad_clip_apply with a coefficient != 1                 8 B
  apply_passing      srk_grad_clip_apply with the coefficient 1 (every workgroup returns at once)
  value              srk_grad_clip_value                                         8 B
  norm_clipping      what a step that clips adds: sumsq + coef + apply           12 B
  norm_passing       what a step that does not clip adds: sumsq + coef + the empty apply    4 B

Every entry is captured into a hipGraph of its own and replayed, which is how the training step runs it; device events around
`--iters` back-to-back replays after a warm-up, median [min, max] of `--repeats` such windows, the entries alternating inside every
repeat.  One JSON line per model.  (Both parameter sets fit the 256 MiB Infinity Cache between iterations: the times are not HBM rates.)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from microbench_lr_sched import captured, compare  # noqa: E402

MODELS = {"edsr_baseline": dict(n_feats=64, n_resblocks=16, res_scale=0.1), "edsr_large": dict(n_feats=256, n_resblocks=32, res_scale=0.1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=7)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_grad_clip.py times GPU launches: no GPU here")
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
        clip = sr_amd.grad_clip.GradClip(opt, 1e9)
        opt.step()                               # the plan and the eager table, outside any capture
        torch.cuda.synchronize()
        t = opt._plans[0].eager
        ema = sr_amd.ema.ParamEMA(ps, 0.999)
        ema.update()
        keep = []

        def entry(names, **state):
            """The launches `names` over the optimizer's table with a clip state of their OWN (the entries alternate: none reads what
            another one wrote), as a function to capture: one graph node per launch, nothing else."""
            st = torch.zeros(L.SRK_CLIP_STATE_FLOATS, device="cuda")
            for k, v in dict(dict(coef=1.0), **state).items():
                st[getattr(L, "SRK_CLIP_" + k.upper())] = v
            args = L.GradClipArgs(**t.pointers(), state=st.data_ptr(), partials=clip.partials.data_ptr(), base=0, nblocks_total=t.nblocks)
            keep.append((st, args))

            def run():
                for name in names:
                    L.call(name, args, torch.cuda.current_stream().cuda_stream)
            return run
        norm = ("srk_grad_sumsq", "srk_grad_clip_coef", "srk_grad_clip_apply")
        # 1 + 2^-23: a multiply that runs on every replay and moves the gradients by 1e-7 per replay.  (A real clip cannot be replayed on
        # the same gradients: after a few replays their norm sits at the threshold and the coefficient is 1.)  norm_clipping is therefore
        # the three launches of a clipping step with the multiply reading that fixed coefficient from a state of its own
        clipping = (entry(norm[:1]), entry(norm[1:2], max_norm=1e9), entry(norm[2:], coef=1.0 + 2.0 ** -23))
        graphs = {
            "ema_update": captured(ema.update),
            "sumsq": captured(entry(norm[:1])),
            "coef": captured(entry(norm[1:2], max_norm=1e9)),
            "apply_clipping": captured(entry(norm[2:], coef=1.0 + 2.0 ** -23)),
            "apply_passing": captured(entry(norm[2:], coef=1.0)),
            "value": captured(entry(("srk_grad_clip_value",), clip_value=1e-3)),
            "norm_clipping": captured(lambda: [fn() for fn in clipping]),
            "norm_passing": captured(entry(norm, max_norm=1e9)),
        }
        torch.cuda.synchronize()
        r = compare({k: g.replay for k, g in graphs.items()}, a.iters, a.repeats)
        n = sum(s.numel() for s in shapes)
        out = {"model": key, "tensors": len(shapes), "parameters": n, "blocks": t.nblocks, "iters": a.iters, "repeats": a.repeats}
        for k, (med, lo, hi) in r.items():
            out[k + "_us"] = round(med, 2)
            out[k + "_min_max_us"] = [round(lo, 2), round(hi, 2)]
        print(json.dumps(out), flush=True)
        del graphs
        clip.detach()


if __name__ == "__main__":
    main()
