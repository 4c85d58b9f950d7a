#!/usr/bin/env python3
"""Train an SR model on the MI355X hot path (flag vocabulary of the reference's train.py:285-303 and of the Trainer
keys its configs use, configs/all.yml:83,125-127).

    python train.py -m edsr --devices 8 --batch_size 16 --max_steps 1000          # 8 ranks, RCCL over xGMI
    python train.py -m srcnn --accelerator cpu --max_steps 2                      # the CPU plumbing case

Data: `--train_dir` (a directory of HR images; LR is synthesised by PIL bicubic like srdata.py:222-231, patches are
drawn and augmented on the GPU by data.PatchSampler, the index space is split over ranks like DistributedSampler) or,
without it, synthetic uniform patches of the BASELINE shape (there is no network for DIV2K here).  `--val_dir`
runs validation_step over full images and prints the per-data-set metric means (on_validation_epoch_end).
`--devices N` with N > 1 starts N processes (one per GPU) through torch.distributed.run unless a launcher already did.
"""
import argparse
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-m", "--model", default="srcnn", help="model name, case-insensitive (models/__init__.py)")
    p.add_argument("-s", "--scale_factor", type=int, default=4)
    p.add_argument("--patch_size", type=int, default=128, help="HR patch edge (LR = patch_size // scale_factor)")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--precision", default="bf16", help="32, 16 or bf16 (Trainer key of the reference)")
    p.add_argument("--losses", default="l1", help="loss or weighted composite, e.g. l1, \"0.9*l1+0.1*flip\", \"0.9*l1+0.1*haarpsi\", \"0.16*l1+0.84*ssim\", \"0.16*l1+0.84*ms_ssim\" (--patch_size >= 161), \"0.9*l1+0.1*gmsd\"; "
                   "the pixel terms charbonnier, huber, smooth_l1, robust (needs --loss_params robust.alpha=... robust.c=...) and psnr, e.g. \"0.5*l1+0.5*charbonnier\"; "
                   "the frequency terms fft (BasicSR's FFTLoss, unnormalised: its weight scales with the patch edge) and ffl (focal frequency loss), e.g. \"l1+0.05*fft\"; "
                   "the perceptual term vgg on a frozen VGG-19 / VGG-16 (needs --loss_params vgg.weights=FILE), e.g. \"l1+0.006*vgg\"")
    p.add_argument("--loss_params", nargs="*", default=[], help="parameters of the pixel losses as <loss>.<key>=<value>, e.g. charbonnier.eps=1e-6 "
                   "huber.delta=0.5 smooth_l1.beta=0.1 robust.alpha=-2 robust.c=0.05 psnr.eps=1e-8; the focal frequency loss takes ffl.alpha=1; "
                   "the VGG loss takes vgg.weights=FILE (required: a torch.load-able state dict of torchvision's vgg19 / vgg16, never downloaded) "
                   "vgg.net=vgg19|vgg16 vgg.layer=relu2_2 vgg.rescale=0.006 vgg.criterion=l2|l1 vgg.precision=32|16|bf16")
    p.add_argument("--metrics", nargs="+", default=None, help="validation metrics (default: the model's, PSNR SSIM); e.g. PSNR SSIM MS-SSIM FLIP GMSD")
    p.add_argument("--optimizer", default="ADAM")
    p.add_argument("--max_steps", type=int, default=100)
    p.add_argument("--max_epochs", type=int, default=-1)
    p.add_argument("--devices", type=int, default=1, help="processes / GPUs on this node (Lightning Trainer key)")
    p.add_argument("--accelerator", default="auto", choices=("auto", "gpu", "cpu"))
    p.add_argument("--strategy", default="ddp", help="accepted for compatibility: data parallel is the only strategy")
    p.add_argument("--default_root_dir", default=".")
    p.add_argument("--checkpoint", default=None, help="state_dict (.pt / Lightning .ckpt) to start from")
    p.add_argument("--save", default=None, help="where rank 0 writes {'state_dict': ...} at the end (with --ema_decay also 'state_dict_ema' and 'ema_num_updates', "
                   "with --lr_schedule also 'lr_schedule', with --gradient_clip_val also 'grad_clip')")
    p.add_argument("--ema_decay", type=float, default=0.0, help="decay of the exponential moving average of the weights, e.g. 0.999 (0: off); "
                   "validation and 'state_dict_ema' use the averaged weights")
    p.add_argument("--lr_schedule", default="", help="learning-rate schedule, advanced once per optimizer step on the device: constant, step, "
                   "multistep, cosine, cosine_restarts (default: none)")
    p.add_argument("--lr_schedule_params", nargs="*", default=[], help="its constants as name=value, e.g. t_max=300000 eta_min=1e-7 "
                   "warmup_steps=2000; step_size=200000 gamma=0.5; milestones=200000,400000 gamma=0.5")
    p.add_argument("--gradient_clip_val", type=float, default=None, help="clip the gradients inside every optimizer step (Lightning Trainer key; "
                   "default: off): the threshold of the total 2-norm, or of each element with --gradient_clip_algorithm value")
    p.add_argument("--gradient_clip_algorithm", default=None, choices=("norm", "value"), help="norm (default) or value (Lightning Trainer key)")
    p.add_argument("--accumulate_grad_batches", type=int, default=1, help="step the optimizer once per this many batches, on the mean of their "
                   "gradients (Lightning Trainer key; default 1: off); --max_steps and --log_every count optimizer steps")
    p.add_argument("--train_dir", default=None, help="directory of HR training images (default: synthetic patches)")
    p.add_argument("--val_dir", default=None, help="directory of HR validation images")
    p.add_argument("--eval_datasets", nargs="+", default=None)
    p.add_argument("--log_every", type=int, default=10)
    p.add_argument("--n_feats", type=int, default=None)
    p.add_argument("--n_resblocks", type=int, default=None)
    p.add_argument("--n_resgroups", type=int, default=None)
    p.add_argument("--res_scale", type=float, default=None)
    return p.parse_args(argv)


def spawn(a):
    """--devices N: N child processes (one per GPU) through torch.distributed.run; nothing has touched the GPU here."""
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.devices}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(cmd, env=env))


def main(argv=None):
    a = parse(argv)
    if a.accumulate_grad_batches < 1:
        raise SystemExit(f"--accumulate_grad_batches {a.accumulate_grad_batches} (must be an integer >= 1)")
    if a.devices > 1 and "WORLD_SIZE" not in os.environ:
        spawn(a)
    import torch
    import sr_amd
    from sr_amd import data as D
    from sr_amd import trainer as T
    names = {m.lower(): m for m in sr_amd.models.__all__ if m != "SRModel"}
    if a.model.lower() not in names:
        raise SystemExit(f"unknown model {a.model!r}; available: {', '.join(sorted(names))}")
    cls = getattr(sr_amd, names[a.model.lower()])
    use_gpu = a.accelerator == "gpu" or (a.accelerator == "auto" and torch.cuda.is_available() and cls is not sr_amd.SRCNN)
    kw = {k: getattr(a, k) for k in ("n_feats", "n_resblocks", "n_resgroups", "res_scale") if getattr(a, k) is not None}
    if a.metrics:
        kw["metrics"] = a.metrics
    if a.eval_datasets:
        kw["eval_datasets"] = a.eval_datasets
    elif a.val_dir:
        kw["eval_datasets"] = [os.path.basename(os.path.normpath(a.val_dir))]
    model = cls(scale_factor=a.scale_factor, patch_size=a.patch_size, batch_size=a.batch_size, precision=a.precision,
                losses=a.losses, optimizer=a.optimizer, default_root_dir=a.default_root_dir, devices=a.devices, ema_decay=a.ema_decay,
                lr_schedule=a.lr_schedule, lr_schedule_params=a.lr_schedule_params, gradient_clip_val=a.gradient_clip_val,
                gradient_clip_algorithm=a.gradient_clip_algorithm, accumulate_grad_batches=a.accumulate_grad_batches,
                loss_params=a.loss_params, **kw)
    sd = None
    if a.checkpoint:
        sd = torch.load(a.checkpoint, map_location="cpu")
        model.load_state_dict(sd.get("state_dict", sd), strict=True)
    if a.lr_schedule and sd is not None and "lr_schedule" in sd:
        model.lr_schedule_state = sd["lr_schedule"]          # the schedule fit() builds continues at the checkpoint's count
    if a.gradient_clip_val is not None and sd is not None and "grad_clip" in sd:
        model.grad_clip_state = sd["grad_clip"]              # the clipper fit() builds continues with the checkpoint's value and counters
    tr = T.Trainer(device="cuda" if use_gpu else "cpu", max_steps=a.max_steps, log_every=a.log_every)
    if a.ema_decay > 0 and sd is not None and "state_dict_ema" in sd:
        # a checkpoint that carries an average restores it (on the device the weights train on); without one fit() starts the
        # average from the loaded weights
        model.to(tr.device)
        model.make_ema().load_state_dict(model, sd["state_dict_ema"], num_updates=sd.get("ema_num_updates"))
    lr_edge = a.patch_size // a.scale_factor

    if a.train_dir:
        pairs, _ = D.load_image_pairs(a.train_dir, a.scale_factor)
        if not use_gpu:
            raise SystemExit("--train_dir draws its patches on the GPU (data.PatchSampler); use synthetic data on CPU")
        sampler = D.PatchSampler(pairs, a.scale_factor, a.patch_size, augment=True, device=tr.device)

        def batches():
            step, epoch = 0, 0
            total = a.max_steps * a.accumulate_grad_batches     # batches: a window of them per optimizer step
            while a.max_steps < 0 or step < total:
                mine = D.shard_indices(len(pairs), tr.rank, tr.world, shuffle=True, seed=0, epoch=epoch)
                for i in range(0, len(mine), a.batch_size):
                    yield sampler.batch(mine[i:i + a.batch_size])
                    step += 1
                    if 0 <= a.max_steps and total <= step:
                        return
                epoch += 1
                if 0 <= a.max_epochs <= epoch:
                    return
        data = batches()
    else:
        n = (a.max_steps if a.max_steps >= 0 else 100) * a.accumulate_grad_batches
        data = (T.synthetic_batch(a.batch_size, 3, lr_edge, a.scale_factor, 1234 + 7919 * s + tr.rank, "cpu") for s in range(n))
    tr.fit(model, data)

    if a.val_dir:
        pairs, stems = D.load_image_pairs(a.val_dir, a.scale_factor)
        mine = D.shard_indices(len(pairs), tr.rank, tr.world, shuffle=False)
        model.eval()
        with torch.no_grad(), model.ema_weights():       # (fit() has flushed: no update is pending)
            for k, i in enumerate(mine):
                lr, hr = pairs[i]
                batch = {"lr": D.image_to_tensor(lr)[None].to(tr.device), "hr": D.image_to_tensor(hr)[None].to(tr.device), "path": [stems[i]]}
                model.validation_step(batch, k, 0)
        metrics = model.on_validation_epoch_end()
        if tr.world > 1:                 # every rank averaged its own shard of the images: combine, weighted by image count
            for k in sorted(metrics):
                t = torch.tensor([float(metrics[k]) * len(mine), float(len(mine))], dtype=torch.float64, device=tr.device)
                torch.distributed.all_reduce(t)
                metrics[k] = t[0] / t[1].clamp_min(1)
        if tr.rank == 0:
            print("validation: " + ", ".join(f"{k} {float(v):.4f}" for k, v in metrics.items()), flush=True)
    if a.save and tr.rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(a.save)), exist_ok=True)
        ckpt = {"state_dict": model.state_dict()}
        if model.ema is not None:
            ckpt["state_dict_ema"] = model.ema.state_dict(model)
            ckpt["ema_num_updates"] = model.ema.num_updates
        sched = getattr(getattr(tr, "optimizer", None), "lr_schedule", None)
        if sched is not None:
            ckpt["lr_schedule"] = sched.state_dict()
        clip = getattr(getattr(tr, "optimizer", None), "_clip", None)
        if clip is not None:
            ckpt["grad_clip"] = clip.state_dict()
        torch.save(ckpt, a.save)
    if tr.rank == 0 and tr.losses:
        print(f"done: {len(tr.losses)} steps, last loss {tr.losses[-1]:.6f}", flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
