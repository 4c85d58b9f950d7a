"""Learning-rate schedules that a replayed training step follows on the device.

The single-launch optimizers (optim.py) take `lr` by value in their launch arguments, so a captured hipGraph replays the learning
rate it was captured with and `trainer.GraphedStep` re-captures when `group["lr"]` changes: a per-iteration schedule would
re-capture every step.  `DeviceLRSchedule` keeps ONE device count and one device double per parameter group instead
(`srk_lr_sched_step`, csrc/lr_sched.hip), makes every group's launch read its learning rate from there when it RUNS (`lr_dev`,
include/srk.h), and issues the launch that advances them behind every `optimizer.step()` -- inside a capture it is a node of the
graph, so every replay counts itself and leaves the next step's learning rate behind.

    lr(t) = warm(t) * main(t)                          t = optimizer steps so far, everything in double
    warm      1 if warmup_steps == 0, else warmup_start + (1 - warmup_start) * min(t, W) / W        LinearLR(warmup_start, 1, W)
    constant  base
    step      base * gamma ** (t // step_size)                                                      StepLR
    multistep base * gamma ** (number of milestones <= t)                                           MultiStepLR
    cosine    eta_min + (base - eta_min) * (1 + cos(pi * t / t_max)) / 2                            CosineAnnealingLR
    cosine_restarts   the same in T_cur / T_i (integer loop over the cycles)                        CosineAnnealingWarmRestarts
    manual    whatever `set_lr()` wrote last: any host-side or per-epoch scheduler drives a replayed step through it

-- torch.optim.lr_scheduler's closed forms (INTEGRATION.md "Learning-rate schedules").  GPU parameters always take the HIP launch
and raise if the library is missing; CPU parameters (SRCNN, the CPU tests) get the same closed forms evaluated on the host into
`group["lr"]`.
"""
import math

import torch

from . import _lib as L
from .optim import _TableStep

_REQUIRED = object()
_INT, _FLOAT, _INTS = "int", "float", "ints"
_WARMUP = {"warmup_steps": (_INT, 0), "warmup_start": (_FLOAT, None)}       # warmup_start: torch's LinearLR default (1/3) with a warm-up, else 1
#: kind -> {constant: (type, default)}; `_REQUIRED`: no default
CONSTANTS = {
    "constant": dict(_WARMUP),
    "step": dict(step_size=(_INT, _REQUIRED), gamma=(_FLOAT, 0.1), **_WARMUP),
    "multistep": dict(milestones=(_INTS, _REQUIRED), gamma=(_FLOAT, 0.1), **_WARMUP),
    "cosine": dict(t_max=(_INT, _REQUIRED), eta_min=(_FLOAT, 0.0), **_WARMUP),
    "cosine_restarts": dict(t_0=(_INT, _REQUIRED), t_mult=(_INT, 1), eta_min=(_FLOAT, 0.0), **_WARMUP),
    "manual": {},
}
_KIND_IDS = {"constant": L.SRK_LR_CONSTANT, "step": L.SRK_LR_STEP, "multistep": L.SRK_LR_MULTISTEP, "cosine": L.SRK_LR_COSINE,
             "cosine_restarts": L.SRK_LR_COSINE_RESTARTS, "manual": L.SRK_LR_CONSTANT}
MAX_MILESTONES = L.SRK_LR_MAX_MILESTONES


def _as_int(name, v):
    if isinstance(v, bool) or (not isinstance(v, int) and not (isinstance(v, float) and v == int(v))):
        raise ValueError(f"lr schedule: {name}={v!r} is not an integer")
    return int(v)


def check_constants(kind, constants):
    """The constants of a schedule of `kind`, defaults filled in and ranges checked (what csrc/lr_sched.hip would refuse is refused
    here first).  ValueError for an unknown kind and for unknown, missing or out-of-range constants."""
    if kind not in CONSTANTS:
        raise ValueError(f"lr schedule kind not recognized: {kind!r}. Supported kinds: {', '.join(CONSTANTS)}")
    spec = CONSTANTS[kind]
    unknown = sorted(set(constants) - set(spec))
    if unknown:
        raise ValueError(f"lr schedule {kind!r} has no constant {', '.join(unknown)} (it takes: {', '.join(spec) or 'none'})")
    out = {}
    for name, (typ, default) in spec.items():
        if name not in constants:
            if default is _REQUIRED:
                raise ValueError(f"lr schedule {kind!r} needs {name}")
            out[name] = default
            continue
        v = constants[name]
        try:
            if typ == _INT:
                out[name] = _as_int(name, v)
            elif typ == _FLOAT:
                out[name] = float(v)
            else:
                out[name] = [_as_int(name, m) for m in v]
        except TypeError:
            raise ValueError(f"lr schedule: {name}={v!r} not understood") from None
    for name in ("step_size", "t_max", "t_0", "t_mult"):
        if name in out and out[name] < 1:
            raise ValueError(f"lr schedule: {name}={out[name]} (must be >= 1)")
    if "milestones" in out:
        ms = out["milestones"]
        if len(ms) > MAX_MILESTONES:
            raise ValueError(f"lr schedule: {len(ms)} milestones (at most {MAX_MILESTONES})")
        if any(a > b for a, b in zip(ms, ms[1:])):
            raise ValueError(f"lr schedule: milestones {ms} are not sorted")
    for name in ("gamma", "eta_min"):
        if name in out and not math.isfinite(out[name]):
            raise ValueError(f"lr schedule: {name}={out[name]}")
    if "warmup_steps" in out:
        if out["warmup_steps"] < 0:
            raise ValueError(f"lr schedule: warmup_steps={out['warmup_steps']} (must be >= 0)")
        if out["warmup_start"] is None:
            out["warmup_start"] = 1.0 / 3 if out["warmup_steps"] > 0 else 1.0
        if not 0.0 < out["warmup_start"] <= 1.0:
            raise ValueError(f"lr schedule: warmup_start={out['warmup_start']} (0 < warmup_start <= 1)")
    return out


def parse_params(kind, params):
    """`name=value` strings -> the constants of `kind`, the way the reference reads `optimizer_params` (models/srmodel.py:603-617):
    `["t_max=300000", "eta_min=1e-7", "warmup_steps=2000"]`; a list is comma-separated (`milestones=200000,400000`).  ValueError for
    a string that is not `name=value`, a value that is not a number, and everything `check_constants` refuses."""
    if kind not in CONSTANTS:
        raise ValueError(f"lr schedule kind not recognized: {kind!r}. Supported kinds: {', '.join(CONSTANTS)}")
    spec, out = CONSTANTS[kind], {}
    for param in params:
        name, sep, value = param.strip().partition("=")
        name, value = name.strip(), value.strip()
        if not sep or not name or not value:
            raise ValueError(f"lr schedule parameter {param!r} is not name=value")
        if name not in spec:
            raise ValueError(f"lr schedule {kind!r} has no constant {name} (it takes: {', '.join(spec) or 'none'})")
        typ = spec[name][0]
        try:
            out[name] = int(value) if typ == _INT else float(value) if typ == _FLOAT else [int(v) for v in value.split(",")]
        except ValueError:
            raise ValueError(f"lr schedule parameter {param!r}: {value!r} is not {'an integer' if typ != _FLOAT else 'a number'}") from None
    return check_constants(kind, out)


def closed_form(kind, c, t, base):
    """lr(t) of a group whose base learning rate is `base`, in double: the device kernel's arithmetic in the same order."""
    if kind == "manual":
        return base
    w = c["warmup_steps"]
    warm = 1.0 if w == 0 else c["warmup_start"] + (1 - c["warmup_start"]) * min(t, w) / w
    if kind == "step":
        main = base * c["gamma"] ** (t // c["step_size"])
    elif kind == "multistep":
        main = base * c["gamma"] ** sum(1 for m in c["milestones"] if m <= t)
    elif kind == "cosine":
        main = c["eta_min"] + (base - c["eta_min"]) * (1 + math.cos(math.pi * t / c["t_max"])) / 2
    elif kind == "cosine_restarts":
        t_cur, t_i = t, c["t_0"]
        if c["t_mult"] == 1:
            t_cur = t % t_i                                  # the loop's result without its t / t_0 iterations
        else:
            while t_cur >= t_i:
                t_cur -= t_i
                t_i *= c["t_mult"]
        main = c["eta_min"] + (base - c["eta_min"]) * (1 + math.cos(math.pi * t_cur / t_i)) / 2
    else:
        main = base
    return warm * main


class DeviceLRSchedule:
    """`DeviceLRSchedule(optimizer, kind, **constants)`: a learning-rate schedule for one of optim.py's optimizers (Adam, Ranger, SGD,
    RMSprop) that advances ONCE PER `optimizer.step()`.

    Every group's current `lr` becomes its base learning rate.  GPU parameters: the count, the groups' learning rates and their bases
    live on the device; every launch of the optimizer reads its group's value when it runs, and one launch of `srk_lr_sched_step`
    (count += 1, lr = f(count)) follows every step from a pair of step hooks (outermost call only, like `trainer.EmaAfterStep`):
    launch by launch, as a node of a hipGraph capture, in `GraphedStep.flush()` / `finish()` and behind `OverlappedGraphStep`'s
    eager step.  The advance is tied to the step that read the old value, so the multi-rank form whose update lags one replay needs
    no extra care.  `group["lr"]` stays at the base value and `trainer.GraphedStep` does not re-capture.  CPU parameters: the same
    closed forms on the host, written into `group["lr"]`.

    A step that `optim.DeviceGradScaler` skips on the device (a non-finite gradient) still advances the schedule: it is a call of
    `step()`.  The torch recipe `scaler.step(opt); scaler.update(); scheduler.step()` does the same.

    get_last_lr()     the groups' current learning rates, computed on the HOST from a mirrored count: no synchronisation.  The
                      mirror follows eager steps and `GraphedStep`'s replays; after replaying a graph of your own that holds a
                      step, tell it with `replayed()`.
    device_lr()       the device values, read back (a synchronisation: tests, logging).
    state_dict() / load_state_dict()   kind, constants, count, base learning rates.  Loading writes the device state (SRK_LR_SET),
                      a captured step follows it.
    set_lr(values)    kind="manual" only: a stream-ordered upload of the groups' learning rates, outside captures; the next step -- a
                      replayed one too -- uses them.
    detach()          removes the hooks; the groups return to the by-value `lr`, at the current value.
    """

    def __init__(self, optimizer, kind, **constants):
        self.constants = check_constants(kind, constants)
        self.kind = kind
        if getattr(optimizer, "lr_schedule", None) is not None:
            raise RuntimeError("this optimizer already has an lr schedule: detach() it first")
        self.optimizer = optimizer
        groups = optimizer.param_groups
        where = {p.device for g in groups for p in g["params"]}
        if len({d.type for d in where}) != 1:
            raise RuntimeError("DeviceLRSchedule: parameters on both CPU and GPU" if where else "DeviceLRSchedule: the optimizer has no parameters")
        self.on_gpu = next(iter(where)).type == "cuda"
        self.base_lrs = [float(g["lr"]) for g in groups]
        self.count = 0                       # host mirror of the device count
        self._depth = 0
        if self.on_gpu:
            if not isinstance(optimizer, _TableStep):
                raise TypeError(f"DeviceLRSchedule needs one of sr_amd.optim's optimizers on the GPU (their launches read lr from the device), got {type(optimizer).__name__}")
            if len(where) != 1:
                raise RuntimeError("DeviceLRSchedule needs all parameters on one device")
            L.load()                         # raises when the library is missing: there is no torch path on the GPU
            self.device = next(iter(where))
            n = len(groups)
            self._state = torch.zeros(2 * n, dtype=torch.float64, device=self.device)        # lr[n] | base_lr[n]
            self._count = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._host = torch.empty(2 * n, dtype=torch.float64, pin_memory=True)
            self._copied = None
            self._upload(self.base_lrs)
            self._launch(L.SRK_LR_SET, 0)
            optimizer._lr_dev = [self._state.data_ptr() + 8 * gi for gi in range(n)]
        else:
            self.device = torch.device("cpu")
            self._apply_host()
        self._handles = (optimizer.register_step_pre_hook(self._pre), optimizer.register_step_post_hook(self._post))
        optimizer.lr_schedule = self

    # -- device state --------------------------------------------------------------------------------
    def _upload(self, values):
        """lr = base_lr = values: one stream-ordered copy from the page-locked staging buffer."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DeviceLRSchedule: learning rates cannot be uploaded inside a hipGraph capture")
        if self._copied is not None:
            self._copied.synchronize()       # the previous values may still be on their way out of the staging buffer
        n = len(values)
        self._host[:n] = torch.tensor(values, dtype=torch.float64)
        self._host[n:] = self._host[:n]
        with torch.cuda.device(self.device):
            self._state.copy_(self._host, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()

    def _launch(self, op, value=0):
        c, n = self.constants, len(self.base_lrs)
        ms = list(c.get("milestones", ()))
        a = L.LrSchedArgs(count=self._count.data_ptr(), lr=self._state.data_ptr(), base_lr=self._state.data_ptr() + 8 * n, ngroups=n,
                          kind=_KIND_IDS[self.kind], op=op, value=int(value),
                          step_size=c.get("step_size", 1), gamma=c.get("gamma", 1.0), nmilestones=len(ms),
                          t_max=c.get("t_max", 1), eta_min=c.get("eta_min", 0.0), t_0=c.get("t_0", 1), t_mult=c.get("t_mult", 1),
                          warmup_steps=c.get("warmup_steps", 0), warmup_start=c.get("warmup_start", 1.0),
                          **{f"m{i}": m for i, m in enumerate(ms)})
        with torch.cuda.device(self.device):
            L.call("srk_lr_sched_step", a, torch.cuda.current_stream().cuda_stream)

    def _apply_host(self):
        for g, lr in zip(self.optimizer.param_groups, self.get_last_lr()):
            g["lr"] = lr

    # -- the advance behind every step ------------------------------------------------------------------
    def _pre(self, optimizer, args, kwargs):
        self._depth += 1

    def _post(self, optimizer, args, kwargs):
        self._depth -= 1
        if self._depth == 0:                 # (the CPU form of optim.py's classes calls torch's own, also wrapped, `step`)
            self.step()

    def step(self):
        """count += 1, lr = f(count).  The hooks call it behind every `optimizer.step()`; there is no need to call it by hand."""
        if self.on_gpu:
            self._launch(L.SRK_LR_ADVANCE)
            if not torch.cuda.is_current_stream_capturing():     # a captured launch runs when the graph is replayed: `replayed()`
                self.count += 1
        else:
            self.count += 1
            self._apply_host()

    def replayed(self, steps=1):
        """Tell the host mirror that a hipGraph holding `steps` optimizer steps has been replayed (`GraphedStep` does)."""
        self.count += int(steps)

    # -- reading ------------------------------------------------------------------------------------------
    def get_last_lr(self):
        return [closed_form(self.kind, self.constants, self.count, b) for b in self.base_lrs]

    def device_lr(self):
        """The learning rates the next step will read, from the device (CPU parameters: from `group["lr"]`)."""
        if not self.on_gpu:
            return [float(g["lr"]) for g in self.optimizer.param_groups]
        return self._state[:len(self.base_lrs)].tolist()

    def device_count(self):
        """The device count (a synchronisation); the host mirror is set to it."""
        if self.on_gpu:
            self.count = int(self._count.item())
        return self.count

    # -- manual ---------------------------------------------------------------------------------------------
    def set_lr(self, values):
        """kind="manual": the groups' learning rates from now on (one number for all groups, or one per group)."""
        if self.kind != "manual":
            raise RuntimeError(f"set_lr() is for kind='manual' (this schedule is {self.kind!r})")
        n = len(self.base_lrs)
        values = [float(values)] * n if isinstance(values, (int, float)) else [float(v) for v in values]
        if len(values) != n:
            raise ValueError(f"set_lr: {len(values)} values for {n} parameter groups")
        if any(not (math.isfinite(v) and v >= 0.0) for v in values):
            raise ValueError(f"set_lr: invalid learning rates {values}")
        if self.on_gpu:
            self._upload(values)
        self.base_lrs = values
        if not self.on_gpu:
            self._apply_host()

    # -- state dict -------------------------------------------------------------------------------------------
    def state_dict(self):
        """(GPU: reads the device count -- with a `GraphedStep` whose update is pending, `flush()` first, as for the weights.)"""
        return {"kind": self.kind, "constants": {k: (list(v) if isinstance(v, list) else v) for k, v in self.constants.items()},
                "count": self.device_count(), "base_lrs": list(self.base_lrs)}

    def load_state_dict(self, sd):
        constants = check_constants(sd["kind"], dict(sd["constants"]))
        bases = [float(b) for b in sd["base_lrs"]]
        if len(bases) != len(self.base_lrs):
            raise ValueError(f"lr schedule state for {len(bases)} parameter groups, the optimizer has {len(self.base_lrs)}")
        count = int(sd["count"])
        if count < 0:
            raise ValueError(f"lr schedule state: count {count}")
        if self.on_gpu:
            self._upload(bases)
        self.kind, self.constants, self.base_lrs, self.count = sd["kind"], constants, bases, count
        if self.on_gpu:
            self._launch(L.SRK_LR_SET, count)
        else:
            self._apply_host()

    def detach(self):
        if self.optimizer is None:
            return
        for h in self._handles:
            h.remove()
        if self.on_gpu:
            self.device_count()
            self.optimizer._lr_dev = None
        self._apply_host()
        self.optimizer.lr_schedule = None
        self.optimizer = None
