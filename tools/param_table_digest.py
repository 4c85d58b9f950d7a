#!/usr/bin/env python3
"""One SHA-256 per configuration over every parameter and state byte a fixed scenario leaves behind: two builds of the library
(`SRK_LIB_PATH=... python tools/param_table_digest.py`, each in a fresh process) compute the same thing iff every line matches.

The scenario walks the table kernels of csrc/optim.hip and csrc/ema.hip over tensors of 1 ... 8193 elements, once with every
tensor in a storage of its own (16-byte accesses) and once as `base[1:]` of a larger one (the scalar path); both go into the one
digest of the configuration.  The configurations are the hyper-parameter lists of tests/test_gpu_optim.py, test_gpu_ranger.py
(at k = 3) and test_gpu_sgd_rmsprop.py for 8 steps each, every optimizer once more under a `DeviceGradScaler` with two parameter
groups and an inf injected at the fourth step, and the four EMA operations."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8193]
STEPS = 8
CONFIGS = (
    [("Adam", kw) for kw in (dict(), dict(lr=3e-2, betas=(0.8, 0.9), eps=1e-6), dict(weight_decay=0.1), dict(maximize=True))]
    + [("Ranger", kw) for kw in (dict(k=3), dict(lr=3e-2, betas=(0.9, 0.99), alpha=0.8, k=3, weight_decay=1e-2))]
    + [("SGD", kw) for kw in (dict(), dict(lr=3e-2, momentum=0.9), dict(lr=3e-2, momentum=0.9, dampening=0.1, weight_decay=1e-2),
                              dict(lr=3e-2, momentum=0.9, nesterov=True, weight_decay=1e-2, maximize=True))]
    + [("RMSprop", kw) for kw in (dict(), dict(lr=1e-3, alpha=0.9, weight_decay=1e-2), dict(momentum=0.9), dict(centered=True),
                                  dict(lr=3e-3, alpha=0.95, eps=1e-6, momentum=0.5, centered=True, weight_decay=1e-2, maximize=True))])
# the two groups of the loss-scaler runs: the configuration with every buffer in use, and a second set of hyper-parameters
SCALED = {"Adam": (dict(lr=1e-2), dict(lr=3e-3, betas=(0.5, 0.9), weight_decay=0.01)),
          "Ranger": (dict(lr=1e-2, k=3), dict(lr=3e-3, betas=(0.9, 0.99), k=3, weight_decay=1e-2)),
          "SGD": (dict(lr=1e-2, momentum=0.9, dampening=0.5), dict(lr=3e-3, momentum=0.8, nesterov=True, weight_decay=1e-2)),
          "RMSprop": (dict(lr=1e-3, momentum=0.9), dict(lr=3e-3, alpha=0.9, centered=True))}


def values(seed, scale_by_index):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) - 0.5) * (10.0 ** (i % 4 - 2) if scale_by_index else 1.0) for i, n in enumerate(SIZES)]


def place(x, aligned):
    if aligned:
        return x.cuda()
    t = torch.empty(x.numel() + 1, device="cuda")[1:]
    t.copy_(x)
    assert t.data_ptr() % 16 == 4
    return t


def feed(h, *tensors):
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())


def feed_optimizer(h, opt, ps):
    for p in ps:
        feed(h, p, *[v for _, v in sorted(opt.state.get(p, {}).items()) if torch.is_tensor(v)])


def run_optimizer(O, name, kw, h):
    for aligned in (True, False):
        ps = [torch.nn.Parameter(place(x, aligned)) for x in values(1, False)]
        opt = getattr(O, name)(ps, **kw)
        for step in range(STEPS):
            for i, (p, g) in enumerate(zip(ps, values(1000 + step, True))):
                p.grad = None if (i == 2 and step in (1, 4)) else place(g, aligned)
            opt.step()
        feed_optimizer(h, opt, ps)


def run_scaled(O, name, h):
    for aligned in (True, False):
        ps = [torch.nn.Parameter(place(x, aligned)) for x in values(2, False)]
        opt = getattr(O, name)([dict(params=ps[:4], **SCALED[name][0]), dict(params=ps[4:], **SCALED[name][1])])
        sc = O.DeviceGradScaler("cuda", init_scale=256.0, growth_interval=3)
        for step in range(STEPS):
            scale = sc.get_scale()
            for p, g in zip(ps, values(2000 + step, True)):
                p.grad = place(g * scale, aligned)
            if step == 3:
                ps[-1].grad[5] = float("inf")
            opt.step(grad_scaler=sc)
        assert sc.skipped_steps == 1
        feed_optimizer(h, opt, ps)
        feed(h, sc.state)


def run_ema(E, decay=0.9):
    """{operation: digest}: every operation's digest covers the parameters and the shadows right after it, in both alignments."""
    hs = {op: hashlib.sha256() for op in ("update", "swap", "store", "load")}
    for aligned in (True, False):
        ps = [place(x, aligned) for x in values(3, False)]
        ema = E.ParamEMA(ps, decay)

        def move(seed):
            for p, d in zip(ps, values(seed, True)):
                p.add_(place(d, aligned))

        for step in range(STEPS):
            move(3000 + step)
            if step == 5:
                ema.set_decay(0.0)                            # w == 1: the shadow becomes the parameter itself
            elif step == 6:
                ema.set_decay(decay)
            ema.update()
            feed(hs["update"], ema.flat)
        feed(hs["update"], *ps)
        assert ema.num_updates == STEPS
        for op, seed in (("swap", 3100), ("store", 3200), ("load", 3300)):
            move(seed)
            getattr(ema, op)()
            feed(hs[op], ema.flat, *ps)
    for op, hh in hs.items():
        print(f"ema {op:48s} {hh.hexdigest()}", flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("param_table_digest.py runs the GPU kernels: no GPU here")
    import sr_amd
    print("library", os.path.basename(sr_amd._lib.LIB_PATH), flush=True)
    with torch.no_grad():
        for name, kw in CONFIGS:
            h = hashlib.sha256()
            run_optimizer(sr_amd.optim, name, kw, h)
            print(f"{name:8s} {str(kw):43s} {h.hexdigest()}", flush=True)
        for name in SCALED:
            h = hashlib.sha256()
            run_scaled(sr_amd.optim, name, h)
            print(f"{name:8s} {'grad scaler, two groups, one inf':43s} {h.hexdigest()}", flush=True)
        run_ema(sr_amd.ema)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
