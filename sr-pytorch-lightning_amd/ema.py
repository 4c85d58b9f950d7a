"""Exponential moving average (EMA) of a model's weights, kept beside the training step.

    s = s + (1 - decay) * (p - s)          after every optimizer step, in fp32, for every floating-point parameter

-- BasicSR's `ema_decay`, timm's `ModelEmaV2`, `torch.optim.swa_utils.get_ema_multi_avg_fn`.  The shadow weights `s` of all tensors
live in ONE flat fp32 buffer and the whole update is ONE launch of `srk_ema_step` (csrc/ema.hip) over a device table of the
parameters, the same table layout the optimizers use (optim.py): RCAN's ~1,600 tensors cost one launch, not the 45 of
`torch._foreach_lerp_`.  The weight 1 - decay and the update count live on the device, so `update()` can be captured into a
hipGraph: replays advance the count and follow `set_decay()` without a re-capture.

To evaluate or save under the average the weights are EXCHANGED IN PLACE (`swap()`, `with ema.swapped():`), never re-pointed: a
captured training step and the packed-weight caches hold the parameters' raw addresses, and `p.data = shadow` would leave them
training and reading memory the model no longer uses (DESIGN.md "EMA of the weights").

GPU parameters always take the HIP kernel and raise if the library is missing.  CPU parameters (SRCNN, the CPU tests) take the same
recurrence in torch ops and swap by value.
"""
import contextlib
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from .optim import _Table


def _weight(decay):
    """w = float32(1 - decay), the difference formed in double."""
    return float(np.float32(1.0 - float(decay)))


class ParamEMA:
    """EMA of `params` (an iterable of tensors; those that are not floating point are ignored, trainable or not makes no difference).

    The shadows start as copies of the parameters' current values, so create it once the model is on its device and any checkpoint
    is loaded.  All parameters must be contiguous fp32 tensors on one device, and their addresses must stay where they are (the
    device table names them): every eager call checks, re-uploads the table if one moved, and raises if that happens inside a
    hipGraph capture.

    update()    s = s + w * (p - s), w = float32(1 - decay); the count advances.  Capturable: no allocation, no host read.
    swap()      exchange weights and shadows in place, bit for bit (twice: everything is back).  Capturable.
    store()     s = p                load()      p = s
    set_decay   a device write: the next update -- a replayed one too -- uses it.
    swapped()   context manager: swap in, run the body, swap back (also when the body raises).

    After `swap()` and `load()` the parameters' `_version` counters advance, so everything cached per weight version (the packed
    weights, MeanShift's folded constants) is rebuilt on the next forward.

    `swap()` exchanges whatever the parameters hold: with a `trainer.GraphedStep` in its multi-rank form the parameters lag one
    update between two calls, so call its `flush()` before `swap()` / `swapped()` / `state_dict()` (as before anything else that
    reads the weights)."""

    def __init__(self, params, decay=0.999):
        self._check_decay(decay)
        seen, ps = set(), []
        for p in params:
            if torch.is_tensor(p) and p.is_floating_point() and id(p) not in seen:
                seen.add(id(p))
                ps.append(p)
        if not ps:
            raise ValueError("ParamEMA: no floating-point parameter to average")
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise RuntimeError("ParamEMA needs contiguous fp32 parameters on one device")
        self.params, self.device, self.on_gpu = ps, dev, dev.type == "cuda"
        self._offsets, off = {}, 0
        for p in ps:
            self._offsets[p] = off
            off += (p.numel() + 3) // 4 * 4                  # every tensor starts 16-byte aligned, as in optim._plan
        self.flat = torch.zeros(max(off, 4), dtype=torch.float32, device=dev)
        self._shadows = [self.flat[self._offsets[p]:self._offsets[p] + p.numel()].view_as(p) for p in ps]
        self._weight = torch.empty(1, dtype=torch.float32, device=dev)
        self._count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.set_decay(decay)
        if self.on_gpu:
            L.load()                                         # raises when the library is missing: there is no torch path on the GPU
            # the optimizers' device table (optim._Table): `g` unused, `state_off` the offset into `flat`.  Made here, outside any
            # capture (page-locked allocations are not capturable); store() below uploads it
            self._table = _Table(_Table.capacity(ps), dev)
        self.store()

    # -- state ------------------------------------------------------------------------------------
    @staticmethod
    def _check_decay(decay):
        if not 0.0 <= float(decay) <= 1.0:                   # (a NaN fails both comparisons)
            raise ValueError(f"Invalid EMA decay: {decay} (0 <= decay <= 1)")

    def set_decay(self, decay):
        self._check_decay(decay)
        self.decay = float(decay)
        self._w = _weight(decay)
        self._weight.fill_(self._w)

    def shadow(self, p):
        """The average of parameter `p`: a view into the flat buffer, shaped like `p`."""
        o = self._offsets[p]
        return self.flat[o:o + p.numel()].view_as(p)

    @property
    def num_updates(self):
        """How many updates the average has had (a host read of the device counter)."""
        return int(self._count.item())

    # -- device table --------------------------------------------------------------------------------
    def _launch(self, op):
        t = self._table
        key = tuple(p.data_ptr() for p in self.params)
        if key != t.key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ParamEMA: a parameter's address moved; the device table cannot be rebuilt inside a hipGraph capture")
            with torch.cuda.device(self.device):
                t.fill([(p, None, self._offsets[p], 0) for p in self.params], key)
            t.copied.synchronize()                           # visible to every stream (a capture runs on a side stream)
        if t.nblocks == 0:                                   # (only empty tensors)
            return
        a = L.EmaArgs(**t.pointers(), shadow=self.flat.data_ptr(), weight=self._weight.data_ptr(), count=self._count.data_ptr(), op=op)
        with torch.cuda.device(self.device):
            L.call("srk_ema_step", a, torch.cuda.current_stream().cuda_stream)
        if op in (L.EMA_SWAP, L.EMA_LOAD):
            # the kernel wrote through raw pointers: tell autograd and every cache keyed on `_version` that the weights changed
            torch.autograd.graph.increment_version(self.params)

    # -- operations ----------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self):
        if self.on_gpu:
            return self._launch(L.EMA_UPDATE)
        if self._w == 1.0:                                   # decay 0: the average is the parameter itself (srk.h)
            torch._foreach_copy_(self._shadows, self.params)
        else:
            torch._foreach_add_(self._shadows, torch._foreach_sub(self.params, self._shadows), alpha=self._w)
        self._count += 1

    @torch.no_grad()
    def swap(self):
        if self.on_gpu:
            return self._launch(L.EMA_SWAP)
        for p, s in zip(self.params, self._shadows):
            t = p.detach().clone()
            p.copy_(s)
            s.copy_(t)

    @torch.no_grad()
    def store(self):
        if self.on_gpu:
            return self._launch(L.EMA_STORE)
        torch._foreach_copy_(self._shadows, self.params)

    @torch.no_grad()
    def load(self):
        if self.on_gpu:
            return self._launch(L.EMA_LOAD)
        torch._foreach_copy_(self.params, self._shadows)

    @contextlib.contextmanager
    def swapped(self):
        """The model runs on the averaged weights inside the block and on the live ones after it.  Do not enter it while a
        `GraphedStep` still has an update pending: `flush()` first."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # -- state dict ----------------------------------------------------------------------------------
    def state_dict(self, model):
        """The averaged weights under `model`'s own parameter names; every other entry (buffers: BatchNorm statistics, ...) is the
        live model's.  `model.load_state_dict` accepts it as it is.  The update count travels as the attribute `num_updates` of
        the returned OrderedDict (the way torch carries `_metadata`), so the mapping holds exactly the model's keys."""
        named = dict(model.named_parameters(remove_duplicate=False))
        live = model.state_dict()
        out = OrderedDict()
        for k, v in live.items():
            p = named.get(k)
            out[k] = (self.shadow(p) if p is not None and p in self._offsets else v).detach().clone()
        if hasattr(live, "_metadata"):
            out._metadata = live._metadata
        out.num_updates = self.num_updates
        return out

    @torch.no_grad()
    def load_state_dict(self, model, sd, num_updates=None):
        """The inverse of `state_dict`: the shadows from `sd`'s entries under `model`'s parameter names (buffers are not touched; the
        live weights neither).  `num_updates`: the count, when `sd` does not carry it."""
        for k, p in model.named_parameters(remove_duplicate=False):
            if p in self._offsets:
                if k not in sd:
                    raise KeyError(f"ParamEMA.load_state_dict: no entry {k!r}")
                self.shadow(p).copy_(sd[k])
        n = getattr(sd, "num_updates", None) if num_updates is None else num_updates
        if n is not None:
            self._count.fill_(int(n))
