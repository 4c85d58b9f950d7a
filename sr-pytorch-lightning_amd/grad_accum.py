"""Gradient accumulation over micro-batches inside the single-launch optimizer step.

Lightning's Trainer key `accumulate_grad_batches` = k lets `.grad` add up over k batches of `loss / k` and steps the optimizer once per
window.  On this stack a user cannot do that by hand: `Trainer.fit` zeroes the gradients and steps once per batch, a replayed hipGraph
holds `optimizer.step()` where no host code can skip it, and the EMA and the lr schedule hang on the optimizer's step hooks.
`GradAccum` attaches to one of optim.py's optimizers instead and adds its launches (csrc/grad_accum.hip) over the device tables the
optimizer builds, with one flat fp32 buffer `acc` per parameter group, laid out like the optimizer's flat state and zero at the start
of a window:

    micro-steps 1 .. k-1   optimizer.accumulate():  SRK_ACCUM_ADD    acc = acc + g                          (no step hook fires)
    micro-step k           optimizer.step():        SRK_ACCUM_FINAL  g = (acc + g) * inv_k;  acc = 0        then clipping, the loss
                           scaler's check, the update, the EMA, the schedule -- once per window, on the mean gradient

`inv_k = float32(1 / k)`, the quotient formed in double.  All fp32, every operation rounded on its own: for k a power of two this is bit
for bit what Lightning computes, for other k it differs by roundings.  Non-finite values are not special-cased: an inf or NaN of any
micro-step reaches the final gradient, where `optim.DeviceGradScaler`'s check skips the whole window's update; FINAL still zeroes `acc`.
The loss scale cannot change inside a window (it is updated only with a real step).  Which of the two launches runs is decided on the
HOST, which keeps the position in the window: a captured hipGraph holds one of them, and `trainer.GraphedStep` keeps one graph per phase.

Two simplifications: the set of tensors that receive a gradient must be the same in every micro-step of a window (RuntimeError
otherwise), and statistics that layers keep per batch (BatchNorm) stay per micro-batch, as under Lightning.

GPU parameters always take the HIP launches and raise if the library is missing; CPU parameters (SRCNN, the CPU tests) take the same
two rules in torch ops on fp32 tensors.
"""
import numpy as np
import torch

from . import _lib as L
from .optim import _TableStep


def check_args(k):
    """`accumulate_grad_batches` as an int, or ValueError: an integer >= 1 (1: off); a bool, a float or a string is refused."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"accumulate_grad_batches={k!r} (must be an integer >= 1)")
    return int(k)


def inv_k(k):
    """float32(1 / k), the quotient formed in double: what SRK_ACCUM_FINAL multiplies by."""
    return float(np.float32(1.0 / k))


class GradAccum:
    """`GradAccum(optimizer, k)`: one of optim.py's optimizers (Adam, Ranger, SGD, RMSprop) steps once per window of k micro-steps, on
    the mean of the window's gradients.  Callers replace `optimizer.step(...)` by `accum.step(...)`.

    step(grad_scaler=None)   the next micro-step: `optimizer.accumulate()` (micro-steps 1 .. k-1) or `optimizer.step(grad_scaler=...)`
                             (micro-step k); returns whether the optimizer stepped.  One table-consuming call, so a hipGraph capture
                             of it needs one `optimizer.reserve_capture_tables()` like a capture of a plain step
    phase                    "accumulate" or "step": what the next call will do
    replayed(n=1)            tell the host position that a captured graph holding n micro-steps has been replayed (under capture the
                             position does not advance: the launches run when the graph does)
    reset()                  drop an incomplete window: acc = 0, position 0 (outside captures)
    detach()                 the optimizer steps on every call again

    The position in the window is a host count; the device holds only `acc`.  The buffers are allocated outside any capture: at the
    first eager use and in `reserve_capture_tables()`."""

    def __init__(self, optimizer, k):
        self.k = check_args(k)
        if not isinstance(optimizer, _TableStep):
            raise TypeError(f"GradAccum needs one of sr_amd.optim's optimizers (its launches run inside their step), got {type(optimizer).__name__}")
        if getattr(optimizer, "_accum", None) is not None:
            raise RuntimeError("this optimizer already has a GradAccum: detach() it first")
        where = {p.device.type for g in optimizer.param_groups for p in g["params"] if p.requires_grad}
        if len(where) != 1:
            raise RuntimeError("GradAccum: parameters on both CPU and GPU" if where else "GradAccum: the optimizer has no trainable parameters")
        self.on_gpu = where == {"cuda"}
        if self.on_gpu:
            L.load()                         # raises when the library is missing: there is no torch path on the GPU
        self.inv_k = inv_k(self.k)
        self.optimizer = optimizer
        self.pos = 0                         # micro-steps of the current window that are in `acc` (host mirror)
        self._acc = {}                       # GPU: group index -> (plan, flat fp32 buffer);  CPU: parameter -> fp32 tensor
        self._ids = {}                       # group index -> identities of the tensors that had a gradient in the window's first micro-step
        optimizer._accum = self

    # -- position ---------------------------------------------------------------------------------------
    @property
    def phase(self):
        return "step" if self.pos >= self.k - 1 else "accumulate"

    def _advance(self, op):
        self.pos = 0 if op == L.SRK_ACCUM_FINAL else self.pos + 1

    def replayed(self, n=1):
        self.pos = (self.pos + int(n)) % self.k

    def step(self, grad_scaler=None):
        final = self.phase == "step"
        if not final:
            self.optimizer.accumulate()
        elif grad_scaler is None:
            self.optimizer.step()
        else:
            self.optimizer.step(grad_scaler=grad_scaler)
        return final

    # -- buffers ----------------------------------------------------------------------------------------
    def _buffer(self, gi, plan):
        have = self._acc.get(gi)
        if have is not None and have[0] is plan:
            return have[1]
        if self.pos != 0:
            raise RuntimeError("GradAccum: a parameter group's plan was rebuilt in the middle of a window (a parameter was added or the "
                               "optimizer state was loaded): finish the window, or reset(), first")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradAccum: the accumulation buffer cannot be allocated inside a hipGraph capture: call "
                               "optimizer.reserve_capture_tables() before it")
        buf = torch.zeros(plan.size, dtype=torch.float32, device=plan.device)
        self._acc[gi] = (plan, buf)
        return buf

    def reserve(self, plans):
        """`reserve_capture_tables()` calls it with the optimizer's plans (group index -> plan), outside any capture."""
        for gi, plan in plans.items():
            self._buffer(gi, plan)

    def acc(self, gi=0):
        """The flat buffer of parameter group `gi` (None before its first use)."""
        have = self._acc.get(gi)
        return have[1] if have is not None else None

    def _same_set(self, gi, ids):
        if self.pos == 0:
            self._ids[gi] = ids
        elif self._ids.get(gi, ids) != ids:
            raise RuntimeError("GradAccum: the set of tensors that receive a gradient changed inside a window of "
                               f"{self.k} micro-steps (micro-step {self.pos + 1}); it must be the same in every micro-step")

    # -- the launches inside optimizer.accumulate() / optimizer.step() --------------------------------------
    def launch(self, launches, op):
        """`_TableStep` calls it with the (group index, plan, table) of every group that has gradients, over the tables it has just
        built: SRK_ACCUM_ADD from `accumulate()`, SRK_ACCUM_FINAL from `step()` before clipping and every check and update."""
        if op == L.SRK_ACCUM_ADD and self.pos >= self.k - 1:
            raise RuntimeError(f"GradAccum: the window of {self.k} micro-steps is full; the next call must be step()")
        seen = {gi for gi, _, _ in launches}
        for gi in self._ids if self.pos else ():
            if gi not in seen and self._ids[gi]:
                self._same_set(gi, ())
        for gi, plan, t in launches:
            self._same_set(gi, t.live_ids)
            buf = self._buffer(gi, plan)
            a = L.GradAccumArgs(**t.pointers(), acc=buf.data_ptr(), inv_k=self.inv_k, op=op)
            with torch.cuda.device(plan.device):
                L.call("srk_grad_accum", a, torch.cuda.current_stream().cuda_stream)
            if op == L.SRK_ACCUM_FINAL:          # the kernel wrote through raw pointers: tell autograd that the gradients changed
                torch.autograd.graph.increment_version(t.grads)
        if self.pos == 0:
            for gi in [g for g in self._ids if g not in seen]:
                del self._ids[gi]
        if not torch.cuda.is_current_stream_capturing():     # a captured launch runs when the graph is replayed: `replayed()`
            self._advance(op)

    @torch.no_grad()
    def apply_cpu(self, op):
        """CPU parameters: the same two rules in torch ops."""
        if op == L.SRK_ACCUM_ADD and self.pos >= self.k - 1:
            raise RuntimeError(f"GradAccum: the window of {self.k} micro-steps is full; the next call must be step()")
        live = [p for g in self.optimizer.param_groups for p in g["params"] if p.requires_grad and p.grad is not None]
        self._same_set(0, tuple(id(p) for p in live))
        for p in live:
            g = p.grad
            if g.is_sparse or g.dtype != torch.float32:
                raise RuntimeError("GradAccum needs dense fp32 gradients")
            acc = self._acc.get(p)
            if acc is None:
                if self.pos != 0:
                    raise RuntimeError("GradAccum: a parameter joined in the middle of a window")
                acc = self._acc[p] = torch.zeros_like(g, memory_format=torch.contiguous_format)
            if op == L.SRK_ACCUM_ADD:
                acc.add_(g)                      # acc = acc + g
            else:
                g.add_(acc).mul_(self.inv_k)     # g = (acc + g) * inv_k  (fp32 addition commutes bit for bit)
                acc.zero_()
        self._advance(op)

    # -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset(self):
        """Drop whatever an incomplete window has accumulated."""
        if self.on_gpu and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradAccum.reset() inside a hipGraph capture")
        for have in self._acc.values():
            (have[1] if isinstance(have, tuple) else have).zero_()
        self.pos = 0
        self._ids = {}

    def detach(self):
        if self.optimizer is None:
            return
        self.optimizer._accum = None
        self.optimizer = None
