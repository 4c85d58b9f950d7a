"""Float64 restatement of the learning-rate schedules (sr_amd.lr_sched, csrc/lr_sched.hip): torch.optim.lr_scheduler's closed forms,

    lr(t) = warm(t) * main(t)

written from the schedulers' `_get_closed_form_lr` (StepLR, MultiStepLR, CosineAnnealingLR), from CosineAnnealingWarmRestarts.step's
integer cycle loop and from LinearLR with end_factor = 1.  tests/test_lr_sched_cpu.py pins them against the torch classes driven step
by step; the CPU and GPU tests compare the product against them."""
import bisect
import math

#: |got - want| <= TOL * base_lr: four orders above double rounding (the worst case of the torch comparisons is 9.4e-15), four below
#: fp32 resolution
TOL = 1e-12


def warm(t, start, steps):
    return 1.0 if steps == 0 else start + (1 - start) * min(t, steps) / steps


def step(t, base, step_size, gamma):
    return base * gamma ** (t // step_size)


def multistep(t, base, milestones, gamma):
    return base * gamma ** bisect.bisect_right(sorted(milestones), t)


def cosine(t, base, t_max, eta_min):
    return eta_min + (base - eta_min) * (1 + math.cos(math.pi * t / t_max)) / 2


def cosine_restarts(t, base, t_0, t_mult, eta_min):
    t_i, t_cur = t_0, t
    while t_cur >= t_i:
        t_cur -= t_i
        t_i *= t_mult
    return eta_min + (base - eta_min) * (1 + math.cos(math.pi * t_cur / t_i)) / 2


def lr(kind, t, base, step_size=1, gamma=0.1, milestones=(), t_max=1, eta_min=0.0, t_0=1, t_mult=1, warmup_steps=0, warmup_start=1.0):
    """The learning rate at count `t` of a group with base learning rate `base`, by the schedule's name in sr_amd.lr_sched."""
    main = {"constant": lambda: base,
            "step": lambda: step(t, base, step_size, gamma),
            "multistep": lambda: multistep(t, base, milestones, gamma),
            "cosine": lambda: cosine(t, base, t_max, eta_min),
            "cosine_restarts": lambda: cosine_restarts(t, base, t_0, t_mult, eta_min)}[kind]()
    return warm(t, warmup_start, warmup_steps) * main
