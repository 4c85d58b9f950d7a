"""Gradient accumulation on two CPU ranks (gloo): `Trainer.fit` with `accumulate_grad_batches` all-reduces every micro-step and runs
SRK_ACCUM_ADD / FINAL behind the reduce (the average of sums is the sum of averages); the replicas end identical and equal one process
that accumulates over the concatenated micro-batches.  Also the optimizer-first order of the multi-rank hipGraph step
(`GraphedStep.shifted_eager_step`), where the micro-step of the pending gradients opens the next call.  Tolerances: tests/test_ddp_gloo.py's."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, WINDOWS = 2, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _full():
    from sr_amd import trainer as T
    return [T.synthetic_batch(4, 3, 16, 2, 400 + s, "cpu") for s in range(K * WINDOWS)]


def _shard(b, rank):
    return {"lr": b["lr"][rank * 2:(rank + 1) * 2], "hr": b["hr"][rank * 2:(rank + 1) * 2], "path": b["path"][rank * 2:(rank + 1) * 2]}


def _worker(rank, world, port, out, form):
    sys.path.insert(0, ROOT)
    os.environ["SRK_USE_TORCH_DDP"] = "0"
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import sr_amd
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = sr_amd.SRCNN(scale_factor=2, optimizer="SGD", accumulate_grad_batches=K, lr_schedule="constant")
    shard = [_shard(b, rank) for b in _full()]
    if form == "fit":
        tr = T.Trainer(device="cpu")
        tr.fit(m, shard)
        opt = tr.optimizer
    else:
        T.init_distributed("cpu")
        opt = m.configure_optimizers()[0]
        gsync = T.GradSync(m, overlap=False, bucket_bytes=4096)
        gsync.broadcast()
        gs = T.GraphedStep(m, m, opt, gsync, warm_steps=0)
        assert gs.segments == 1 and gs.accum is opt._accum
        for i, sh in enumerate(shard):
            gs.shifted_eager_step(sh)
            assert gs.pending and opt._accum.pos == i % K and opt.lr_schedule.count == i // K     # (this batch's micro-step is still pending)
        gs.finish()
        assert not gs.pending
        gsync.detach()
    assert opt._accum.pos == 0 and opt.lr_schedule.count == WINDOWS
    torch.save({k: v.clone() for k, v in m.state_dict().items()}, os.path.join(out, f"r{rank}.pt"))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("form", ["fit", "shifted"])
def test_two_ranks_accumulate_like_a_single_process(tmp_path, form):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), form), nprocs=2, join=True)
    a, b = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    for k in a:
        assert torch.equal(a[k], b[k]), f"replicas diverged at {k}"
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(v, None)
    import sr_amd
    from sr_amd import trainer as T
    torch.manual_seed(0)
    m = sr_amd.SRCNN(scale_factor=2, optimizer="SGD", accumulate_grad_batches=K)
    start = {k: v.clone() for k, v in m.state_dict().items()}
    T.Trainer(device="cpu").fit(m, _full())
    for k, v in m.state_dict().items():
        assert torch.allclose(v, a[k], rtol=1e-5, atol=1e-7), k
    assert any(not torch.equal(v, start[k]) for k, v in m.state_dict().items())
