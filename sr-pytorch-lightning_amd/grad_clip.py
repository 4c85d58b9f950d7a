"""Gradient clipping by norm and by value inside the single-launch optimizer step.

Lightning's Trainer keys `gradient_clip_val` / `gradient_clip_algorithm` (the reference's configs/all.yml, `trainer:` block) call
`torch.nn.utils.clip_grad_norm_` / `clip_grad_value_` between backward and `optimizer.step()`.  On this stack that place does not
exist for a user: a replayed hipGraph runs no host code between the two, `torch.nn.utils.clip_grad_norm_` over a few hundred tensors is
hundreds of small launches, and under `optim.DeviceGradScaler` the gradients still carry the loss scale when the optimizer sees them.
`GradClip` attaches to one of optim.py's optimizers instead and adds its launches (csrc/grad_clip.hip) to `step()` itself, over the
device tables that step has just built:

    norm    srk_grad_sumsq per group, srk_grad_clip_coef once, srk_grad_clip_apply per group:
            total_norm = sqrt(sum of g^2 over ALL groups) / loss scale;  coef = min(1, clip_val / (total_norm + 1e-6));  g *= coef
    value   srk_grad_clip_value per group:  g = clamp(g, -b, b),  b = clip_val (times the loss scale under the scaler)

-- torch's formulas, the sums in double.  The thresholds, the last norm and coefficient and two counters live on the device: a
captured step recomputes them on every replay and follows `set_clip_val()` without a re-capture.  Two deliberate differences from
torch (INTEGRATION.md "Gradient clipping"): a norm that is not finite leaves the gradients as they are (coef = 1, counted in
`num_nonfinite`) where torch multiplies every gradient by NaN; and under the scaler `p.grad` holds the clipped gradient still
multiplied by the loss scale.

GPU parameters always take the HIP launches and raise if the library is missing; CPU parameters (SRCNN, the CPU tests) go through
`torch.nn.utils.clip_grad_norm_` / `clip_grad_value_` themselves.
"""
import math

import torch

from . import _lib as L
from .optim import _CHUNK, _TableStep

ALGORITHMS = ("norm", "value")


def check_args(clip_val, algorithm):
    """(clip_val as a float, algorithm) or ValueError: `algorithm` is Lightning's "norm" or "value", `clip_val` a number > 0."""
    if algorithm not in ALGORITHMS:
        raise ValueError(f"gradient_clip_algorithm not recognized: {algorithm!r}. Supported: {', '.join(ALGORITHMS)}")
    if isinstance(clip_val, bool) or not isinstance(clip_val, (int, float)) or not (math.isfinite(clip_val) and clip_val > 0):
        raise ValueError(f"gradient_clip_val={clip_val!r} (must be a finite number > 0)")
    return float(clip_val), algorithm


class GradClip:
    """`GradClip(optimizer, clip_val, algorithm="norm")`: clip the gradients of one of optim.py's optimizers (Adam, Ranger, SGD, RMSprop)
    inside every `optimizer.step()` -- launch by launch, as nodes of a hipGraph capture, in `GraphedStep.flush()` / `finish()` and behind
    `OverlappedGraphStep`'s eager step; always after `GradSync`'s average, so every rank clips the same gradients.

    The norm is taken over all parameter groups of the optimizer, like `clip_grad_norm_(model.parameters())`.  The gradients are
    clipped in place: after the step `p.grad` is the clipped gradient (under `optim.DeviceGradScaler`: clipped and still scaled).

    total_norm, coef   0-d views of the device state: the last step's norm (of the unscaled gradients) and coefficient; no host read
    stats()            one host read: total_norm, coef, num_clipped (steps with coef < 1), num_nonfinite (steps whose norm was not finite)
    set_clip_val(v)    a device write: the next step -- a replayed one too -- uses it
    state_dict() / load_state_dict()   the algorithm, the value and the two counters
    detach()           the optimizer steps without clipping again
    """

    def __init__(self, optimizer, clip_val, algorithm="norm", norm_type=2.0, foreach=None):
        self.clip_val, self.algorithm = check_args(clip_val, algorithm)
        if float(norm_type) != 2.0:
            raise NotImplementedError(f"norm_type={norm_type} is not implemented by GradClip (the device norm is the 2-norm)")
        if foreach is not None:
            raise NotImplementedError("foreach is not implemented by GradClip (one launch walks every tensor already)")
        if not isinstance(optimizer, _TableStep):
            raise TypeError(f"GradClip needs one of sr_amd.optim's optimizers (its launches run inside their step), got {type(optimizer).__name__}")
        if optimizer._clip is not None:
            raise RuntimeError("this optimizer already has a GradClip: detach() it first")
        params = [p for g in optimizer.param_groups for p in g["params"] if p.requires_grad]
        where = {p.device for p in params}
        if len(where) != 1:
            raise RuntimeError("GradClip needs all parameters on one device" if where else "GradClip: the optimizer has no trainable parameters")
        self.device = next(iter(where))
        self.on_gpu = self.device.type == "cuda"
        self.optimizer = optimizer
        # SRK_CLIP_*: max_norm, clip_value, total_norm, coef, num_clipped, num_nonfinite (csrc/grad_clip.hip reads and writes them)
        self.state = torch.zeros(L.SRK_CLIP_STATE_FLOATS, dtype=torch.float32, device=self.device)
        self.state[L.SRK_CLIP_COEF] = 1.0
        self._write_threshold()
        if self.on_gpu:
            L.load()                         # raises when the library is missing: there is no torch path on the GPU
            # one double per table block over all groups, sized for "every parameter has a gradient" (allocated here, outside any capture)
            self._capacity = sum((p.numel() + _CHUNK - 1) // _CHUNK for p in params)
            self.partials = torch.zeros(max(self._capacity, 1), dtype=torch.float64, device=self.device)
        optimizer._clip = self

    # -- device state --------------------------------------------------------------------------------
    def _write_threshold(self):
        if self.on_gpu and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradClip: the threshold cannot be written inside a hipGraph capture (a replay reads it from the device)")
        self.state[L.SRK_CLIP_MAX_NORM] = self.clip_val if self.algorithm == "norm" else 0.0
        self.state[L.SRK_CLIP_CLIP_VALUE] = self.clip_val if self.algorithm == "value" else 0.0

    def set_clip_val(self, clip_val):
        """The threshold from now on (stream-ordered device writes, outside captures)."""
        self.clip_val, _ = check_args(clip_val, self.algorithm)
        self._write_threshold()

    @property
    def total_norm(self):
        return self.state[L.SRK_CLIP_TOTAL_NORM]

    @property
    def coef(self):
        return self.state[L.SRK_CLIP_COEF]

    def stats(self):
        s = self.state.tolist()
        return {"total_norm": s[L.SRK_CLIP_TOTAL_NORM], "coef": s[L.SRK_CLIP_COEF], "num_clipped": int(s[L.SRK_CLIP_NUM_CLIPPED]),
                "num_nonfinite": int(s[L.SRK_CLIP_NUM_NONFINITE])}

    # -- the launches inside optimizer.step() -----------------------------------------------------------
    def launch(self, launches, grad_scaler):
        """`_TableStep.step()` calls it with the (plan, table, arguments) of every group it is about to update, before its own launches:
        the tables are the ones the step built (nothing is built or uploaded here)."""
        if not launches:
            return
        total = sum(t.nblocks for _, t, _ in launches)
        if total > self._capacity or any(plan.device != self.device for plan, _, _ in launches):
            raise RuntimeError("GradClip: the optimizer's parameters changed after the clipper was attached; detach() it and attach a new one")
        scaler = grad_scaler.state.data_ptr() if grad_scaler is not None else None
        args, base = [], 0
        for _, t, _ in launches:
            args.append(L.GradClipArgs(**t.pointers(), state=self.state.data_ptr(), partials=self.partials.data_ptr(), base=base,
                                       nblocks_total=total, scaler_state=scaler))
            base += t.nblocks
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            if self.algorithm == "norm":
                for a in args:
                    L.call("srk_grad_sumsq", a, stream)
                L.call("srk_grad_clip_coef", args[0], stream)
                for a in args:
                    L.call("srk_grad_clip_apply", a, stream)
            else:
                for a in args:
                    L.call("srk_grad_clip_value", a, stream)
        for _, t, _ in launches:             # the kernels wrote through raw pointers: tell autograd that the gradients changed
            torch.autograd.graph.increment_version(t.grads)

    @torch.no_grad()
    def clip_cpu(self):
        """CPU parameters: torch's own functions over the groups' parameters (so a non-finite norm behaves as torch's does there)."""
        params = [p for g in self.optimizer.param_groups for p in g["params"] if p.grad is not None]
        if not params:
            return
        if self.algorithm == "value":
            torch.nn.utils.clip_grad_value_(params, self.clip_val)
            return
        norm = float(torch.nn.utils.clip_grad_norm_(params, self.clip_val))
        c = self.clip_val / (norm + 1e-6)
        self.state[L.SRK_CLIP_TOTAL_NORM], self.state[L.SRK_CLIP_COEF] = norm, (1.0 if c > 1.0 else c)     # what torch multiplied by
        if not math.isfinite(norm):
            self.state[L.SRK_CLIP_NUM_NONFINITE] += 1.0
        elif c < 1.0:
            self.state[L.SRK_CLIP_NUM_CLIPPED] += 1.0

    # -- state dict ------------------------------------------------------------------------------------
    def state_dict(self):
        """(one host read; with a `GraphedStep` whose update is pending, `flush()` first, as for the weights)"""
        s = self.stats()
        return {"algorithm": self.algorithm, "clip_val": self.clip_val, "num_clipped": s["num_clipped"], "num_nonfinite": s["num_nonfinite"]}

    def load_state_dict(self, sd):
        self.clip_val, self.algorithm = check_args(sd["clip_val"], sd["algorithm"])
        self._write_threshold()
        self.state[L.SRK_CLIP_NUM_CLIPPED] = float(int(sd.get("num_clipped", 0)))
        self.state[L.SRK_CLIP_NUM_NONFINITE] = float(int(sd.get("num_nonfinite", 0)))

    def detach(self):
        if self.optimizer is None:
            return
        self.optimizer._clip = None
        self.optimizer = None
