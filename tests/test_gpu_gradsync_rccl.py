"""GradSync's bucketed gradient mean over RCCL (one rank on the GPU box)."""


import json


import math


import os


import socket


import subprocess


import sys


import numpy as np


import pytest


import torch


import torch.nn.functional as F


from oracle import fill, functional as OF


pytestmark = pytest.mark.gpu


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))


# srresnet_full_x4 is judged against the float64 oracle instead (test_srresnet_fullsize_backward_vs_float64_oracle): with
# 33 BatchNorm layers over 288 pixels its gradients are ill-conditioned -- the reference's own fp32 result is 4 % (relative
# L2, worst tensor) away from the float64 value of the same expression
LARGE = sorted(k for k, v in MANIFEST.items() if v["class"] != "SRCNN" and v["n_params_trainable"] >= 1_000_000 and k != "srresnet_full_x4")


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    return sr_amd


# ---------------------------------------------------------------------------------------------------------------
# PSNR within 0.01 dB of the reference path
# ---------------------------------------------------------------------------------------------------------------
def smooth_images(n, size, seed):
    """Smooth synthetic 'photographs': sums of low-frequency sin*cos products per channel plus a little noise, in [0,1]."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, size), torch.linspace(0, 1, size), indexing="ij")
    out = torch.zeros(n, 3, size, size)
    for i in range(n):
        for c in range(3):
            img = torch.zeros(size, size)
            for _ in range(6):
                fx, fy = (torch.rand(2, generator=g) * 9 + 0.5).tolist()
                px, py = (torch.rand(2, generator=g) * 6.28).tolist()
                amp = float(torch.rand(1, generator=g)) * 0.25
                img += amp * torch.sin(6.28 * fx * xx + px) * torch.cos(6.28 * fy * yy + py)
            out[i, c] = 0.5 + img
    out += 0.01 * torch.randn(out.shape, generator=g)
    return out.clamp(0, 1)


def psnr(a, b):
    mse = ((a.double().clamp(0, 1) - b.double().clamp(0, 1)) ** 2).flatten(1).mean(1)
    return float((10.0 * torch.log10(1.0 / (mse + 1e-12))).mean())


@pytest.fixture(scope="module")
def trained_edsr(A):
    """EDSR-baseline x4 trained for 300 Adam steps (bf16 HIP path) on smooth 192x192 images, bicubic LR."""
    kw = dict(n_feats=64, n_resblocks=16, res_scale=0.1, scale_factor=4)
    torch.manual_seed(0)
    m = A.EDSR(precision="bf16", **kw).cuda()
    hr = smooth_images(48, 192, 11)
    lr = F.interpolate(hr, scale_factor=0.25, mode="bicubic", antialias=True).clamp(0, 1)
    hr_d, lr_d = hr.cuda(), lr.cuda()
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)      # the reference's effective optimizer
    g = torch.Generator().manual_seed(1)
    first = last = None
    for step in range(300):
        idx = torch.randint(0, 48, (16,), generator=g).cuda()
        opt.zero_grad(set_to_none=True)
        loss = m.training_step({"lr": lr_d[idx], "hr": hr_d[idx]}, step)["loss"]
        loss.backward()
        opt.step()
        first = float(loss) if first is None else first
        last = float(loss)
    assert math.isfinite(last) and last < 0.5 * first, (first, last)
    sd = {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items()}
    hr_t = smooth_images(6, 192, 99)
    lr_t = F.interpolate(hr_t, scale_factor=0.25, mode="bicubic", antialias=True).clamp(0, 1)
    with torch.no_grad():
        y_ref = OF.forward("EDSR", sd, lr_t, **kw)
    return kw, sd, lr_t, hr_t, y_ref


# ---------------------------------------------------------------------------------------------------------------
# two models alternating in one process (BASELINE configs[4])
# ---------------------------------------------------------------------------------------------------------------
def _steps(A, cls, kw, batches, other=None):
    torch.manual_seed(0)
    m = getattr(A, cls)(precision=16, **kw).cuda()
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4, fused=True)
    losses = []
    for b in batches:
        opt.zero_grad(set_to_none=True)
        loss = m.training_step(b, 0)["loss"]
        (loss * 128.0).backward()
        for p in m.parameters():
            if p.grad is not None:
                p.grad.mul_(1.0 / 128.0)
        opt.step()
        losses.append(float(loss))
        if other is not None:
            other()
    return losses, {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------
# RCCL path: GradSync on a 1-rank nccl group (2 ranks when there are 2 GPUs)
# ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


DDP_WORKER = r"""
import os, sys, torch
sys.path.insert(0, {root!r})
import sr_amd
from sr_amd import trainer as T
rank, world, local = T.init_distributed("cuda", force=True)
dev = torch.device("cuda", local)
torch.manual_seed(0)
mode = {mode!r}
m = sr_amd.EDSR(n_feats=64, n_resblocks=4 if mode == "segments" else 2, res_scale=0.1, scale_factor=2, precision="bf16").to(dev)
g = torch.Generator().manual_seed(5)
full = [{{"lr": torch.rand(4, 3, 24, 24, generator=g), "hr": torch.rand(4, 3, 48, 48, generator=g)}} for _ in range(6)]
per = 4 // world
gs = T.GradSync(m, overlap=(mode != "pack_reduce"), bucket_bytes=64 << 10)
gs.broadcast()
opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, fused=True)
if mode == "graphed":
    # the trainer's loop: eager steps with the overlapped all-reduces, then forward + backward + packing as one hipGraph, the
    # all-reduce issued eagerly, the optimizer step (the one-launch HIP Adam) as a second graph
    opt = m.configure_optimizers()[0]
    gstep = T.GraphedStep(m, m, opt, gs, warm_steps=2)
    for b in full:
        gstep({{k: v[rank * per:(rank + 1) * per].to(dev) for k, v in b.items()}})
    assert gstep.graphs is not None and len(gstep.graphs) == 2 and not gstep.failed
    gstep.finish()          # (the last replay's update: the multi-rank graph opens with the optimizer step of the previous one)
    full = []
if mode == "segments":
    # large-model form: the backward pass as three graph segments with the bucket all-reduces issued between them
    os.environ["SRK_DDP_SEGMENTS"] = "3"
    opt = m.configure_optimizers()[0]
    gstep = T.GraphedStep(m, m, opt, gs, warm_steps=2)
    for b in full:
        gstep({{k: v[rank * per:(rank + 1) * per].to(dev) for k, v in b.items()}})
    assert gstep.ogs is not None and gstep.ogs.nseg == 3 and len(gstep.graphs) == 4 and not gstep.failed, (gstep.ogs and gstep.ogs.nseg, gstep.failed)
    assert len(gstep.ogs.gsync.group_buckets) >= 3 and all(gstep.ogs.gsync.group_buckets[k] for k in range(3))
    full = []
for b in full:
    sh = {{k: v[rank * per:(rank + 1) * per].to(dev) for k, v in b.items()}}
    opt.zero_grad(set_to_none=True)
    m._calculate_losses(img_sr=m(sh["lr"]), img_hr=sh["hr"])["loss"].backward()
    if mode == "hooks":
        gs.sync()
    else:
        gs.pack(); gs.reduce()
    assert all(p.grad.data_ptr() == gs.views[p].data_ptr() for p in gs.params)
    opt.step()
torch.cuda.synchronize()
torch.save({{k: v.float().cpu() for k, v in m.state_dict().items()}}, os.path.join({out!r}, f"{{mode}}_r{{rank}}.pt"))
torch.distributed.barrier()
torch.distributed.destroy_process_group()
"""


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["hooks", "pack_reduce", "graphed", "segments"])
def test_gradsync_over_rccl(A, tmp_path, mode):
    """A HIP EDSR trains 6 steps under trainer.GradSync on an `nccl` (= RCCL) process group: 1 rank always (the
    collective path itself), 2 ranks when the box has 2 GPUs (replica equality).  The result must equal the same
    steps without any process group (global batch)."""
    ngpu = torch.cuda.device_count()
    world = 2 if ngpu >= 2 else 1
    script = tmp_path / "worker.py"
    script.write_text(DDP_WORKER.format(root=ROOT, mode=mode, out=str(tmp_path)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=800, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    sds = [torch.load(tmp_path / f"{mode}_r{r}.pt") for r in range(world)]
    for k in sds[0]:
        for s in sds[1:]:
            assert torch.equal(sds[0][k], s[k]), f"replicas diverged at {k}"
    # the same three steps in this process, no process group
    torch.manual_seed(0)
    m = A.EDSR(n_feats=64, n_resblocks=4 if mode == "segments" else 2, res_scale=0.1, scale_factor=2, precision="bf16").cuda()
    g = torch.Generator().manual_seed(5)
    full = [{"lr": torch.rand(4, 3, 24, 24, generator=g), "hr": torch.rand(4, 3, 48, 48, generator=g)} for _ in range(6)]
    opt = m.configure_optimizers()[0] if mode in ("graphed", "segments") else torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, fused=True)
    for b in full:
        opt.zero_grad(set_to_none=True)
        m._calculate_losses(img_sr=m(b["lr"].cuda()), img_hr=b["hr"].cuda())["loss"].backward()
        opt.step()
    for k, v in m.state_dict().items():
        dv = (v.float().cpu() - sds[0][k]).abs()
        if mode in ("graphed", "segments"):
            # replayed steps vs launch-by-launch steps.  The bound dates from the fp32 weight gradient's float atomics, under which Adam's
            # lr-sized moves on near-zero gradients let single weights part by a few steps' worth; the gradients are reproducible now
            # (tests/test_gpu_step_reproducible.py), this multi-rank bound is kept as it was
            assert float(dv.max()) <= 6.5e-3 and float(dv.mean()) <= 3e-4, (k, float(dv.max()), float(dv.mean()))
        else:
            assert float(dv.max()) <= (2e-6 if world == 1 else 2e-4) * max(1.0, float(v.abs().max())), (k, float(dv.max()))
