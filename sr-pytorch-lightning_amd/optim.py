"""Optimizers of the training hot path on the HIP kernels.

`Adam` is torch.optim.Adam -- the optimizer the reference builds (models/srmodel.py:57-64 `_supported_optimizers['ADAM']`,
:145-154 `configure_optimizers`, always at torch's defaults because :602-603 drops the user's parameters) -- with the whole
update as ONE launch of `srk_adam_step` (csrc/optim.hip) instead of one launch per few dozen tensors.  Same constructor,
same `state_dict()` layout (`step`, `exp_avg`, `exp_avg_sq` per parameter), same arithmetic in fp32.  The step count lives
on the device, so `step()` can be captured into a hipGraph and replayed.

`Ranger` is torch_optimizer 0.3.0's `Ranger` (RAdam + Lookahead; the reference's `_supported_optimizers['Ranger']`) on the same
table and the same kind of single launch, `srk_ranger_step`.

`SGD` and `RMSprop` are torch.optim.SGD / torch.optim.RMSprop (`_supported_optimizers['SGD']` / `['RMSprop']`) on the same table:
`srk_sgd_step`, `srk_rmsprop_step`.  Same constructors, `state_dict()` interchangeable with torch's in both directions.

All four take `lr` by value in their launch arguments (a tensor `lr` is refused); `lr_sched.DeviceLRSchedule` makes their launches read
it from the device instead (`lr_dev`), so that a replayed step follows a schedule.

Nothing here falls back to PyTorch arithmetic: parameters must be fp32 tensors on a GPU and the HIP library must load.
"""
import ctypes as C
import math

import torch

from . import _lib as L

_CHUNK = 4096           # elements per workgroup (256 threads x 4 x float4)


class DeviceGradScaler:
    """Dynamic loss scaling whose state lives on the GPU: torch.amp.GradScaler's arithmetic (init_scale 2^16, growth factor 2,
    backoff 0.5, growth interval 2000 -- what Lightning's "16-mixed" precision wraps around the reference's training_step for
    `precision: 16`, configs/all.yml:122) without its per-step host read.  GradScaler.step() asks the HOST whether a gradient was
    non-finite and then calls or skips optimizer.step() from Python; a hipGraph replay cannot branch on the host, so fp16 training
    ran launch by launch (RCAN: 72.8 ms per step against 19 ms replayed).  Here the check, the skip and the scale update are
    launches of the step itself (`srk_adam_step_scaled`, `srk_loss_scale_update`):

        loss_s = scaler.scale(loss)            # loss * scale (a device scalar: the backward pass carries it)
        loss_s.backward()
        optimizer.step(grad_scaler=scaler)     # non-finite gradient anywhere -> nothing is updated; scale halves; else g / scale

    state (8 device floats): scale, growth tracker, found_inf, growth factor, backoff factor, growth interval, skipped steps, -."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.state = torch.tensor([init_scale, 0.0, 0.0, growth_factor, backoff_factor, float(growth_interval), 0.0, 0.0],
                                  dtype=torch.float32, device=device)

    def scale(self, loss):
        return loss * self.state[0]            # a view of the state: no host read, capturable

    def get_scale(self):
        return float(self.state[0])            # (host read: logging only)

    @property
    def skipped_steps(self):
        return int(self.state[6])

    def state_dict(self):
        return {"scale": self.get_scale(), "growth_tracker": int(self.state[1])}

    def load_state_dict(self, d):
        self.state[0] = float(d["scale"])
        self.state[1] = float(d.get("growth_tracker", 0))


class _Table:
    """One device copy of a parameter table -- slots | 16-byte gap | blocks (srk_adam_slot / srk_adam_block) -- with its page-locked
    staging buffer: what every table kernel reads (csrc/param_table.h).  The eager optimizer steps own one and every hipGraph
    capture gets ITS OWN (a captured upload is a memcpy node that re-reads the staging buffer on every replay, so nothing an eager
    step does later may touch the bytes a live graph points at: ADVICE r2); `ema.ParamEMA` owns one."""

    def __init__(self, cap, dev):
        self.table = torch.empty(cap, dtype=torch.uint8, device=dev)   # device bytes
        self.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        self.copied = None      # event behind the last eager upload from `host`
        self.key = None
        self.grads = None       # the gradient tensors the table was built for (kept alive: their addresses are in it)
        self.live = []          # the parameters in the table
        self.live_ids = None    # their identities (same set, moved addresses: only the pointer fields are rewritten)
        self.slots = None
        self.nslots = self.nblocks = self.blocks_off = 0

    @staticmethod
    def capacity(params):
        """Bytes of the table that holds all of `params`."""
        return C.sizeof(L.AdamSlot) * len(params) + 16 + C.sizeof(L.AdamBlock) * sum((p.numel() + _CHUNK - 1) // _CHUNK for p in params)

    def fill(self, entries, key, capturing=False):
        """`entries`: (parameter, gradient or None, offset into the flat state buffers, index of its count) per tensor, in table
        order; `key`: what the caller compares to decide that the table is stale.  Slots and blocks (one tensor per block of at most
        _CHUNK elements) are rebuilt when the SET of parameters changed; otherwise only the pointer fields are rewritten.  Then one
        host-to-device copy from the staging buffer, which was sized when the table was made (so nothing is allocated here):
        captured into a hipGraph it is ONE memcpy node that replays the same bytes."""
        ids = tuple(id(p) for p, _, _, _ in entries)
        same_set = ids == self.live_ids                      # only addresses moved (eager steps re-allocate the gradients)
        if not same_set:
            self.slots = (L.AdamSlot * max(len(entries), 1))()
            blocks = []
            for i, (p, _, off, idx) in enumerate(entries):
                n = p.numel()
                self.slots[i].state_off, self.slots[i].n, self.slots[i].step_idx = off, n, idx
                for s0 in range(0, n, _CHUNK):
                    blocks.append((i, min(_CHUNK, n - s0), s0))
            barr = (L.AdamBlock * max(len(blocks), 1))()
            for j, (i, cnt, s0) in enumerate(blocks):
                barr[j].slot, barr[j].count, barr[j].start = i, cnt, s0
            self.nblocks = len(blocks)
        slots = self.slots
        for i, (p, g, _, _) in enumerate(entries):
            slots[i].p, slots[i].g = p.data_ptr(), (g.data_ptr() if g is not None else None)
        ssz = C.sizeof(L.AdamSlot) * len(entries)
        boff = (ssz + 15) // 16 * 16
        total = boff + C.sizeof(L.AdamBlock) * self.nblocks
        upto = total if not same_set else ssz                # the block list depends on the sizes only
        if upto:
            assert total <= self.host.numel()
            if self.copied is not None and not capturing:
                self.copied.synchronize()                    # the previous table may still be on its way out of `host`
            C.memmove(self.host.data_ptr(), C.addressof(slots), ssz)
            if not same_set:
                C.memmove(self.host.data_ptr() + boff, C.addressof(barr), total - boff)
            self.table[:upto].copy_(self.host[:upto], non_blocking=True)
            if not capturing:
                self.copied = torch.cuda.Event()
                self.copied.record()
        self.key, self.live_ids = key, ids
        self.grads, self.live = [g for _, g, _, _ in entries], [p for p, _, _, _ in entries]
        self.nslots, self.blocks_off = len(entries), boff
        return self

    def pointers(self):
        """(slots, blocks, nslots, nblocks): the first four fields of every table kernel's arguments."""
        return dict(slots=self.table.data_ptr(), blocks=self.table.data_ptr() + self.blocks_off, nslots=self.nslots, nblocks=self.nblocks)


class _Plan:
    """Per parameter group: flat state buffers, the device step counter and the device tables of (parameter, gradient)."""

    def __init__(self):
        self.offsets = {}       # param -> offset (floats) into the flat state buffers
        self.index = {}         # param -> index into `steps`
        self.keys = ()          # the state keys the group's configuration uses (`_TableStep._keys`)
        self.flat = {}          # state key -> flat buffer of every tensor's values (exp_avg, exp_avg_sq[, slow_buffer])
        self.m = self.v = None  # flat["exp_avg"], flat["exp_avg_sq"] (Adam, Ranger)
        self.device = None
        self.steps = self.ticket = None  # per-parameter update counts (torch counts per parameter)
        self.cap = 0
        self.size = 0           # floats of every flat buffer (what `grad_accum.GradAccum` sizes its own by)
        self.eager = None       # _Table of the launch-by-launch steps
        self.captured = []      # _Tables owned by hipGraph captures: written once, kept alive as long as the plan
        self.spare = None       # allocated OUTSIDE any capture (page-locked allocations are not capturable) for the next one


class _TableStep:
    """What the single-launch optimizers share: per parameter group a `_Plan` (flat state buffers, device step counts, the
    device tables of (parameter, gradient)), the capture bookkeeping and the launches (one group; several groups under a
    `DeviceGradScaler`: every check first).  The subclass names its flat state (`_flat_keys`, or `_keys(group)` where it depends on
    the group's hyper-parameters), its entry points (`_entry`: <entry>_step, _step_scaled, _check_scaled, _update_scaled), its
    launch arguments (`_args`) and its CPU form (`_cpu_step`).  `_step_key`: the state key the device count is published under
    (None: the count is internal)."""

    _flat_keys = ("exp_avg", "exp_avg_sq")
    _step_key = "step"
    _entry = "srk_adam"
    _sparse_msg = "Adam does not support sparse gradients, please consider SparseAdam instead"
    #: per parameter group the address of the device double its launches read `lr` from (`lr_dev`, include/srk.h), set by
    #: `lr_sched.DeviceLRSchedule`; None: `lr` travels by value from `group["lr"]`
    _lr_dev = None
    #: the `lr_sched.DeviceLRSchedule` attached to this optimizer, if any
    lr_schedule = None
    #: the `grad_clip.GradClip` attached to this optimizer, if any: `step()` issues its launches over the tables it has just built
    _clip = None
    #: the `grad_accum.GradAccum` attached to this optimizer, if any: `accumulate()` adds the gradients to its buffers, `step()` turns them
    #: into the window's mean before anything else reads them
    _accum = None

    # -- state ------------------------------------------------------------------------------------
    def _keys(self, group):
        """The flat state buffers the group's configuration uses (nothing else is allocated, read or written)."""
        return self._flat_keys

    def _count0(self, st, carried):
        """The number of updates a tensor has had when a plan adopts it (`st`: its state; `carried`: its count in the plan this one
        is rebuilt from, or None)."""
        return float(st.get("step", 0) or 0)                 # (an int or a tensor)

    def _plan(self, gi, group):
        plan = self._plans.get(gi)
        params = [p for p in group["params"] if p.requires_grad]
        keys = tuple(self._keys(group))
        if plan is not None and plan.keys == keys and all(p in plan.offsets for p in params):
            return plan
        if not params:
            return None
        old = plan                                           # rebuilt: a parameter was added, or a hyper-parameter changed the keys
        dev = params[0].device
        for p in params:
            if not p.is_cuda:
                raise RuntimeError("sr-pytorch-lightning_amd.optim.%s runs on the GPU only (parameters are on %s); there is no CPU path" % (type(self).__name__, p.device))
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise RuntimeError("HIP %s needs contiguous fp32 parameters on one device" % type(self).__name__)
        plan = _Plan()
        off = 0
        for k, p in enumerate(params):
            plan.offsets[p], plan.index[p] = off, k
            off += (p.numel() + 3) // 4 * 4                 # every tensor starts 16-byte aligned
        plan.keys, plan.device, plan.size = keys, dev, max(off, 4)
        plan.flat = {key: torch.zeros(plan.size, dtype=torch.float32, device=dev) for key in keys}
        plan.m, plan.v = plan.flat.get("exp_avg"), plan.flat.get("exp_avg_sq")
        plan.steps = torch.zeros(len(params), dtype=torch.float32, device=dev)
        plan.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        cap = plan.cap = _Table.capacity(params)             # the largest case: every parameter has a gradient
        plan.eager, plan.spare = _Table(cap, dev), _Table(cap, dev)
        host_steps = [0.0] * len(params)
        old_counts = old.steps.tolist() if old is not None else []
        for k, p in enumerate(params):
            if not keys and self._step_key is None and p not in self.state:
                continue                                     # stateless (SGD without momentum): torch keeps no entry either
            st = self.state[p]
            o, n = plan.offsets[p], p.numel()
            views = {key: buf[o:o + n].view_as(p) for key, buf in plan.flat.items()}
            for key, view in views.items():                  # loaded (load_state_dict) or carried-over (a rebuilt plan) state
                if torch.is_tensor(st.get(key)):
                    view.copy_(st[key])
            host_steps[k] = self._count0(st, old_counts[old.index[p]] if old is not None and p in old.index else None)
            st.update(views)
            if self._step_key is not None:
                st[self._step_key] = plan.steps[k]
        if any(host_steps):
            plan.steps.copy_(torch.tensor(host_steps, dtype=torch.float32))
        self._plans[gi] = plan
        return plan

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}                                     # re-adopt the loaded moments into flat buffers at the next step

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_plans"):
            self._plans.pop(len(self.param_groups) - 1, None)

    # -- capture bookkeeping ---------------------------------------------------------------------------
    def reserve_capture_tables(self):
        """Call OUTSIDE a capture, right before one: every plan gets the table (device bytes + page-locked staging buffer) the
        capture will own.  Page-locked allocations (hipHostMalloc) are not capturable, and a capture consumes the spare without
        a non-capturing step in between to refill it (a re-capture after an lr change in the single-process form, where the
        optimizer step lives inside the graph)."""
        for gi, group in enumerate(self.param_groups):
            plan = self._plan(gi, group)
            if plan is not None and plan.spare is None:
                plan.spare = _Table(plan.cap, plan.device)
        if self._accum is not None:
            self._accum.reserve(self._plans)

    def release_captured_tables(self):
        """Call after the graphs that captured this optimizer's step have been destroyed (a re-capture): their tables are
        unreferenced bytes from then on."""
        for plan in self._plans.values():
            plan.captured = []

    # -- device table --------------------------------------------------------------------------------
    def _table(self, plan, group):
        """The table this step's launch reads: the eager one (rebuilt / re-pointed when gradient addresses moved), or a
        fresh one owned by the capture in progress."""
        live = [(p, p.grad) for p in group["params"] if p.requires_grad and p.grad is not None]
        key = tuple((p.data_ptr(), g.data_ptr(), g.numel()) for p, g in live)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            # owned by this capture and never rewritten: eager steps between replays (a short last batch, validation-time
            # fallbacks) keep using `plan.eager`
            # (no spare: the caller did not `reserve_capture_tables()`; the page-locked allocation below only succeeds in a
            # relaxed-mode capture)
            t, plan.spare = (plan.spare or _Table(plan.cap, plan.device)), None
            plan.captured.append(t)
        else:
            t = plan.eager
            if plan.spare is None:
                plan.spare = _Table(plan.cap, plan.device)
            if key == t.key:
                return t
        for p, g in live:
            if g.is_sparse:
                raise RuntimeError(self._sparse_msg)
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or g.numel() != p.numel():
                raise RuntimeError("HIP %s needs contiguous fp32 gradients on the parameter's device" % type(self).__name__)
        return t.fill([(p, g, plan.offsets[p], plan.index[p]) for p, g in live], key, capturing)

    # -- step -------------------------------------------------------------------------------------
    def _launches(self):
        """(group index, plan, table, launch arguments) of every parameter group that has gradients: the device tables of this call
        (`_table`: the eager one, or a fresh one owned by the capture in progress) and what the group's update is launched with."""
        launches = []
        lr_dev = self._lr_dev
        if lr_dev is not None and len(lr_dev) != len(self.param_groups):
            raise RuntimeError("%s: a parameter group was added after the lr schedule was attached; detach() it and attach a new one" % type(self).__name__)
        for gi, group in enumerate(self.param_groups):
            plan = self._plan(gi, group)
            if plan is None:
                continue
            with torch.cuda.device(plan.device):
                t = self._table(plan, group)
                if t.nblocks == 0:
                    continue
                a = self._args(plan, t, group)
                if lr_dev is not None:
                    a.lr_dev = lr_dev[gi]                    # read when the launch runs: a replay follows the schedule
                launches.append((gi, plan, t, a))
        return launches

    @torch.no_grad()
    def accumulate(self):
        """A micro-step that is not the last of its window (`grad_accum.GradAccum`): the gradients are added to the accumulator's
        buffers over the same tables `step()` builds, and nothing else happens -- it is not `step()`, so no step hook fires (the EMA and
        the lr schedule stay where they are), nothing is clipped, checked or updated."""
        if self._accum is None:
            raise RuntimeError("%s.accumulate() needs a grad_accum.GradAccum attached" % type(self).__name__)
        on_gpu = {p.is_cuda for group in self.param_groups for p in group["params"]}
        if on_gpu == {False}:
            return self._accum.apply_cpu(L.SRK_ACCUM_ADD)
        if on_gpu != {True}:
            raise RuntimeError("%s: parameters on both CPU and GPU" % type(self).__name__)
        self._accum.launch([(gi, plan, t) for gi, plan, t, _ in self._launches()], L.SRK_ACCUM_ADD)

    @torch.no_grad()
    def step(self, closure=None, grad_scaler=None):
        """grad_scaler: a `DeviceGradScaler` whose scale the gradients still carry (fp16 training): the launch checks them for
        non-finite values, skips the whole update if it finds one, divides by the scale otherwise, and adjusts the scale.
        With a `grad_clip.GradClip` attached the gradients of all groups are clipped first, in place, by launches of this call; with a
        `grad_accum.GradAccum` they are first of all replaced by the mean over the window this call ends (SRK_ACCUM_FINAL)."""
        on_gpu = {p.is_cuda for group in self.param_groups for p in group["params"]}
        if on_gpu == {False}:
            if grad_scaler is not None:
                raise RuntimeError("DeviceGradScaler needs GPU parameters")
            if self._clip is None and self._accum is None:
                return self._cpu_step(closure)
            loss = None
            if closure is not None:                          # the closure produces the gradients: it runs before they are averaged and clipped
                with torch.enable_grad():
                    loss = closure()
            if self._accum is not None:
                self._accum.apply_cpu(L.SRK_ACCUM_FINAL)
            if self._clip is not None:
                self._clip.clip_cpu()
            self._cpu_step(None)
            return loss
        if on_gpu != {True}:
            raise RuntimeError("%s: parameters on both CPU and GPU" % type(self).__name__)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        launches = self._launches()
        if self._accum is not None:                          # the window's mean gradient, in place: before clipping and every check and update
            self._accum.launch([(gi, plan, t) for gi, plan, t, _ in launches], L.SRK_ACCUM_FINAL)
        launches = [(plan, t, a) for _, plan, t, a in launches]
        if self._clip is not None:
            self._clip.launch(launches, grad_scaler)         # over the tables built above: before every check and update
        lib, e = L.load(), self._entry
        # torch.amp.GradScaler.step looks at EVERY group's gradients before it steps any: with several groups all checks come first
        # (an inf in group 1 used to leave group 0 updated); one group keeps the combined entry point (same three launches)
        split = grad_scaler is not None and len(launches) > 1
        if split:
            for plan, t, a in launches:
                with torch.cuda.device(plan.device):
                    L.check(getattr(lib, e + "_check_scaled")(C.byref(a), grad_scaler.state.data_ptr(), torch.cuda.current_stream().cuda_stream), e + "_check_scaled")
        for plan, t, a in launches:
            with torch.cuda.device(plan.device):
                stream = torch.cuda.current_stream().cuda_stream
                if grad_scaler is None:
                    L.call(e + "_step", a, stream)
                elif split:
                    L.check(getattr(lib, e + "_update_scaled")(C.byref(a), grad_scaler.state.data_ptr(), stream), e + "_update_scaled")
                else:
                    L.check(getattr(lib, e + "_step_scaled")(C.byref(a), grad_scaler.state.data_ptr(), stream), e + "_step_scaled")
                # the kernel wrote through raw pointers: tell autograd (and the packed-weight cache, which keys on it) that
                # the parameters changed, as an in-place torch op would
                torch.autograd.graph.increment_version(t.live)
        if grad_scaler is not None:
            with torch.cuda.device(grad_scaler.state.device):
                L.check(lib.srk_loss_scale_update(grad_scaler.state.data_ptr(), torch.cuda.current_stream().cuda_stream), "srk_loss_scale_update")
        return loss


class Adam(_TableStep, torch.optim.Adam):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay, amsgrad) with a single-launch step for GPU parameters.

    `amsgrad=True` is not implemented (the reference never sets it); `maximize` and L2 `weight_decay` are.  A model whose
    parameters live on the CPU (SRCNN, the reference's CPU-runnable case, runs on torch ops there) steps through
    torch.optim.Adam itself; GPU parameters always take the HIP kernel and raise if the library is missing."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise NotImplementedError("amsgrad is not implemented by the HIP Adam (the reference never enables it)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize)
        self._plans = {}

    def _args(self, plan, t, group):
        b1, b2 = group["betas"]
        return L.AdamArgs(**t.pointers(),
                          m=plan.m.data_ptr(), v=plan.v.data_ptr(), steps=plan.steps.data_ptr(), ticket=plan.ticket.data_ptr(),
                          lr=float(group["lr"]), beta1=float(b1), beta2=float(b2), eps=float(group["eps"]),
                          weight_decay=float(group["weight_decay"]), maximize=int(bool(group["maximize"])),
                          one_minus_beta1=1.0 - float(b1), one_minus_beta2=1.0 - float(b2))

    def _cpu_step(self, closure):
        return torch.optim.Adam.step(self, closure)


def _reject_unsupported(name, lr, differentiable, fused=None):
    if isinstance(lr, torch.Tensor):
        raise NotImplementedError(f"a tensor lr is not implemented by the HIP {name} (the launch takes lr by value)")
    if differentiable:
        raise NotImplementedError(f"differentiable=True is not implemented by the HIP {name}")
    if fused:
        raise NotImplementedError(f"fused=True is not implemented by the HIP {name} (its step is one HIP launch already)")


class SGD(_TableStep, torch.optim.SGD):
    """torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov, maximize=...) with a single-launch step
    (`srk_sgd_step`) for GPU parameters.  torch's constructor and its validation; `foreach` is accepted and has no effect on the
    GPU; `differentiable=True`, `fused=True` and a tensor `lr` raise NotImplementedError.

    State: none with `momentum == 0` (12 B of traffic per parameter), else `momentum_buffer` (20 B) -- torch's keys, and a
    `state_dict()` that loads into torch.optim.SGD and back.  torch creates a tensor's `momentum_buffer` as a copy of the first
    gradient it ever receives, ignoring `dampening`; "has this tensor had a step" is a per-tensor count ON THE DEVICE (so a
    replayed hipGraph and a step skipped by the loss scaler get it right) that never appears in `state` or `state_dict()`.
    The buffers are views into one flat buffer: `opt.state[p]["momentum_buffer"]` is a live tensor from the first GPU step of
    the optimizer on, and its content is MEANINGLESS until `p` has had its own first step; `state_dict()` exports None for such
    a tensor (it reads the counts on the host: not on the step's path), and `load_state_dict` sets the count to 1 where it is
    given a tensor and to 0 where it finds None or nothing.

    CPU parameters step through torch.optim.SGD.step itself."""

    _step_key = None
    _entry = "srk_sgd"
    _sparse_msg = "sr-pytorch-lightning_amd.optim.SGD does not support sparse gradients"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        _reject_unsupported("SGD", lr, differentiable, fused)
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         maximize=maximize, foreach=foreach, differentiable=False, fused=fused)
        self._plans = {}

    def _keys(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _count0(self, st, carried):
        if carried is not None:
            return carried
        return 1.0 if torch.is_tensor(st.get("momentum_buffer")) else 0.0    # loaded: torch has a buffer from the first step on

    def state_dict(self):
        sd = super().state_dict()
        idx = 0
        for gi, group in enumerate(self.param_groups):
            plan = self._plans.get(gi)
            counts = plan.steps.tolist() if plan is not None and plan.keys else None
            for p in group["params"]:
                if counts is not None and p in plan.index and counts[plan.index[p]] == 0 and idx in sd["state"]:
                    sd["state"][idx] = dict(sd["state"][idx], momentum_buffer=None)      # torch: no buffer before the first step
                idx += 1
        return sd

    def _args(self, plan, t, group):
        mom = float(group["momentum"])
        return L.SgdArgs(**t.pointers(),
                         buf=plan.flat["momentum_buffer"].data_ptr() if mom != 0 else None, steps=plan.steps.data_ptr(),
                         lr=float(group["lr"]), momentum=mom, dampening=float(group["dampening"]),
                         weight_decay=float(group["weight_decay"]), nesterov=int(bool(group["nesterov"])),
                         maximize=int(bool(group["maximize"])))

    def _cpu_step(self, closure):
        for group in self.param_groups:
            if any(p.grad is not None and p.grad.is_sparse for p in group["params"]):
                raise RuntimeError(self._sparse_msg)
        return torch.optim.SGD.step(self, closure)


class RMSprop(_TableStep, torch.optim.RMSprop):
    """torch.optim.RMSprop(params, lr, alpha, eps, weight_decay, momentum, centered, ...) with a single-launch step
    (`srk_rmsprop_step`) for GPU parameters.  torch's constructor and its validation; `capturable` / `foreach` are accepted and
    have no effect on the GPU (the step count always lives on the device); `differentiable=True` and a tensor `lr` raise
    NotImplementedError.

    State: torch's keys for the configuration -- `step`, `square_avg`, `momentum_buffer` iff `momentum > 0`, `grad_avg` iff
    `centered` -- as views into flat buffers; only those buffers exist and are touched (20 B of traffic per parameter, +8 B with
    momentum, +8 B centered).  `state_dict()` loads into torch.optim.RMSprop and back; `load_state_dict` takes CPU tensors and
    integer or tensor steps.  CPU parameters step through torch.optim.RMSprop.step itself."""

    _entry = "srk_rmsprop"
    _sparse_msg = "RMSprop does not support sparse gradients"

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False):
        _reject_unsupported("RMSprop", lr, differentiable)
        super().__init__(params, lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=centered,
                         capturable=capturable, foreach=foreach, maximize=maximize, differentiable=False)
        self._plans = {}

    def _keys(self, group):
        return ("square_avg",) + (("momentum_buffer",) if group["momentum"] > 0 else ()) + (("grad_avg",) if group["centered"] else ())

    def _args(self, plan, t, group):
        ptr = {key: buf.data_ptr() for key, buf in plan.flat.items()}
        return L.RmspropArgs(**t.pointers(),
                             sq=ptr["square_avg"], buf=ptr.get("momentum_buffer"), ga=ptr.get("grad_avg"), steps=plan.steps.data_ptr(),
                             lr=float(group["lr"]), alpha=float(group["alpha"]), eps=float(group["eps"]),
                             weight_decay=float(group["weight_decay"]), momentum=float(group["momentum"]),
                             centered=int(bool(group["centered"])), maximize=int(bool(group["maximize"])))

    def _cpu_step(self, closure):
        return torch.optim.RMSprop.step(self, closure)



def ranger_scalars(t, beta1, beta2, n_sma_threshhold):
    """(rectified, step size) of a tensor's t-th Ranger step, in double: torch_optimizer's RAdam scalars (srk.h has the rule)."""
    b2t = beta2 ** t
    n_max = 2 / (1 - beta2) - 1
    n_sma = n_max - 2 * t * b2t / (1 - b2t)
    if n_sma > n_sma_threshhold:
        return True, math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - beta1 ** t)
    return False, 1.0 / (1 - beta1 ** t)


class Ranger(_TableStep, torch.optim.Optimizer):
    """torch_optimizer.Ranger (0.3.0: RAdam + Lookahead) with a single-launch step for GPU parameters.

    Same constructor, same group keys (`N_sma_threshhold` spelled as there), same per-parameter state (`step`, `exp_avg`,
    `exp_avg_sq`, `slow_buffer`).  One deliberate difference: the package caches RAdam's (N_sma, step size) per step count in a
    buffer shared by ALL groups, so a second group with other betas reuses the first group's scalars; here every tensor's
    scalars come from its own group (the same numbers whenever the groups share betas).  A model whose parameters live on the
    CPU steps through a plain-torch fp32 form of the same rule; GPU parameters always take `srk_ranger_step`."""

    _flat_keys = ("exp_avg", "exp_avg_sq", "slow_buffer")
    _entry = "srk_ranger"
    _sparse_msg = "Ranger optimizer does not support sparse gradients"

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0):
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid eps: {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._plans = {}

    def _args(self, plan, t, group):
        b1, b2 = group["betas"]
        return L.RangerArgs(**t.pointers(),
                            m=plan.m.data_ptr(), v=plan.v.data_ptr(), slow=plan.flat["slow_buffer"].data_ptr(),
                            steps=plan.steps.data_ptr(), lr=float(group["lr"]), beta1=float(b1), beta2=float(b2),
                            alpha=float(group["alpha"]), n_sma_threshold=float(group["N_sma_threshhold"]), eps=float(group["eps"]),
                            weight_decay=float(group["weight_decay"]), k=int(group["k"]))

    def _cpu_step(self, closure):
        """The package's step in torch fp32 ops (CPU parameters), with the scalars of each tensor's own group."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            lr, wd, thr = group["lr"], group["weight_decay"], group["N_sma_threshhold"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError(self._sparse_msg)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                    st["slow_buffer"] = p.detach().clone()
                m, v = st["exp_avg"], st["exp_avg_sq"]
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                m.mul_(b1).add_(g, alpha=1 - b1)
                t = st["step"] = int(st["step"]) + 1
                rect, s = ranger_scalars(t, b1, b2, thr)
                if wd != 0:
                    p.add_(p, alpha=-wd * lr)
                if rect:
                    p.addcdiv_(m, v.sqrt().add_(group["eps"]), value=-s * lr)
                else:
                    p.add_(m, alpha=-s * lr)
                if t % group["k"] == 0:
                    slow = st["slow_buffer"]
                    slow.add_(p - slow, alpha=group["alpha"])
                    p.copy_(slow)
        return loss
