"""Where each parameter's gradient goes: the deferred (grouped) weight-gradient queue, the per-parameter routing record, and `route`,
which every producer of a parameter gradient asks.  Part of `ops` (re-exported there).

A producer states what it can take -- accumulate into an existing fp32 `.grad`, write trainer.GradSync's flat-buffer slice, share
one tensor between the uses of a parameter in one pass -- and gets the tensor to write into, whether its kernel accumulates, and
(through `Route.hand`) what its backward hands autograd.  The decisions per producer:

| producer | existing fp32 `.grad` | GradSync slice | second use in one pass |
|---|---|---|---|
| queued 3x3 16-bit conv (`wgrad`: Conv, ConvChain, ResTrunk, RCAB, TailConv, WDSR-B `w3`) | finalize accumulates, autograd gets None | written there on the pass's first use | accumulate round into the first job's buffers while it is queued |
| immediate conv (`wgrad` fallback) | fresh, autograd adds | written there on the pass's first use | fresh |
| HeadConv / SkipConv (`wgrad_raw` direct) | fresh | not used | fresh |
| HrTail | fresh | written there (fp32 params) | fresh |
| Proj weight / bias | accumulate | written there | fresh |
| PReLU slope, Proj slope | accumulate | not used | fresh |
| BatchNorm / BNPReLU gamma, beta, slope | accumulate | not used | added into the first use's tensor, autograd gets None |
| RCAB channel-attention params (`defer_rowsum`) | eager sum | not used | queued row sums flushed now, eager sum |
| WDSR-B pointwise pair | fresh | not used | fresh |

Parameters with tensor hooks (and post-accumulate hooks that do not flush the queue) cannot be filled after their producer's backward
returns (`Route.late` False): a conv job takes the immediate row, BatchNorm a fresh tensor.  WeightNormGroup's effective weights are
not leaves but stay queued: its backward flushes the queue before it reads them.

The state behind these decisions lives in ONE record per parameter (`_Record`, the tensor's only routing attribute).  It answers two
different questions with two different keys, on purpose:
  * is the first use's job still in the queue?  -- the queue generation `_WQ.gen`, bumped by every flush or discard (WeightNormGroup's
    flush in the middle of a pass included) and only then;
  * is this the same autograd pass?  -- the graph-task id of the running backward call, which changes with every backward call, each
    segment of `backward_segments` included.
"""
import contextlib
import ctypes as C
import weakref

import torch

from . import _lib as L
from .ops import _DT, _batch_chunks, _knob, _need_gpu, _pitch, _ptr, _roundup, _stream      # (ops.py imports this module at its END: these exist by then)

__all__ = ["Route", "route", "set_slice", "set_flush_aware", "mark_proxy", "forget", "wgrad_raw", "wgrad", "hold_wgrads",
           "hold_wgrads_discard", "set_defer_wgrad", "flush_wgrads", "discard_wgrads", "defer_rowsum", "TableHolder", "static_tables",
           "graph_capture"]


# --------------------------------------------------------------------------------------------
# the per-parameter record
# --------------------------------------------------------------------------------------------
class _Record:
    """Routing state of one parameter (or WeightNormGroup proxy), kept as `p.__dict__["_srk_route"]`.

    slice       GradSync's flat-buffer slice for the gradient (set_slice), or None
    flush_aware its post-accumulate hook flushes the queue before reading the gradient (set_flush_aware)
    proxy       a WeightNormGroup effective weight: not a leaf, queued all the same (mark_proxy)
    job         (queue generation, dw address, db address) of its queued conv job
    rowsum_gen  queue generation of its queued row-sum job
    slice_pass  graph-task id of the pass that got the slice
    first       (graph-task id, weakref) of the tensor the pass's first use handed autograd (`route(share=True)`)"""
    slice = job = rowsum_gen = slice_pass = first = None
    flush_aware = proxy = False


def _rec(p, create=False):
    r = p.__dict__.get("_srk_route")
    if r is None and create:
        r = p.__dict__["_srk_route"] = _Record()
    return r


def set_slice(p, view):
    """trainer.GradSync: write the gradient of `p` into `view` (a slice of its flat buffer), see `_take_slice`."""
    _rec(p, True).slice = view


def set_flush_aware(p, on):
    """trainer.GradSync: the post-accumulate hook on `p` flushes the deferred queue before it reads the gradient."""
    _rec(p, True).flush_aware = bool(on)


def mark_proxy(w):
    """WeightNormGroup: `w` is an effective weight whose consumer (the group's backward) flushes the queue before reading its gradient."""
    _rec(w, True).proxy = True


def forget(p):
    """Drop all routing state of `p` (GradSync.detach)."""
    p.__dict__.pop("_srk_route", None)


def _pass_id():
    f = getattr(torch._C, "_current_graph_task_id", None)
    return f() if f is not None else -1


def _late(p, shape):
    """(may the gradient of `p` be filled after its producer's backward has returned, its existing fp32 `.grad` to accumulate into or None)."""
    if p is None:
        return True, None
    r = _rec(p)
    if r is not None and r.proxy:
        return True, None
    if not (p.is_leaf and p.requires_grad):
        return False, None
    if getattr(p, "_backward_hooks", None):
        return False, None                      # a tensor hook reads the gradient inside backward
    if getattr(p, "_post_accumulate_grad_hooks", None) and not (r is not None and r.flush_aware):
        return False, None
    g = p.grad
    if g is None:
        return True, None
    if g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == tuple(shape) and g.is_cuda:
        return True, g
    return False, None


def _take_slice(p, shape, dev):
    """GradSync's slice for the gradient of `p`, or None.  GradSync keeps all gradients in one flat fp32 buffer (what the bucket
    all-reduces run on): a kernel that writes the slice directly saves the per-step pack copy, and autograd adopts a view of it as
    `.grad`.  Only while `p` has no gradient yet, and only for the FIRST use of `p` in a backward pass: `.grad` stays None until
    AccumulateGrad has seen every use, so a second use would overwrite the first one's result in the same memory and autograd would
    then add two aliases of it (2 g_last instead of g_1 + g_2)."""
    if p is None or not p.is_leaf or p.grad is not None:
        return None
    r = _rec(p)
    t = r.slice if r is not None else None
    if t is None or tuple(t.shape) != tuple(shape) or t.device != dev:
        return None
    pid = _pass_id()
    if pid >= 0:
        if r.slice_pass == pid:
            return None
        r.slice_pass = pid
    return t.detach()           # a fresh tensor object on the same memory (AccumulateGrad adopts a gradient nobody else references)


class Route:
    """What `route` decided for one parameter gradient.  out: the tensor the kernel writes (acc False) or adds into (acc True), or None
    (the kernel's own fresh output); late: the gradient may be filled after the producer's backward has returned."""
    __slots__ = ("out", "acc", "late", "want", "_first_of")

    def hand(self, t):
        """What backward returns to autograd for the parameter, `t` being what the kernel produced (`out` when it was given)."""
        if self.acc or not self.want:
            return None
        if self._first_of is not None:
            _rec(self._first_of, True).first = (_pass_id(), weakref.ref(t))
        return t


def route(p, shape, dev=None, *, accumulate=False, slice=False, share=False, buffer=False, want=True):
    """Where the gradient of parameter `p` (shape `shape`, on `dev`) goes.  What the producer can take, in the order tried: accumulate --
    add into an existing fp32 `.grad`;  slice -- write GradSync's slice;  share -- a second use in the same autograd pass adds into the
    tensor the first use handed autograd (a BatchNorm used twice, SRResNet's ResBlock: no add launch of autograd's).  Otherwise a fresh
    tensor, allocated here with `buffer`, else the kernel's own output.  want=False: no gradient wanted (hand() gives None)."""
    r = Route()
    r.out, r.acc, r.want, r._first_of = None, False, want, None
    if not want:
        r.late = True
        return r
    r.late, g = _late(p, shape)
    if accumulate and g is not None:
        r.out, r.acc = g, True
    elif slice and (t := _take_slice(p, shape, dev)) is not None:
        r.out = t
    elif share and r.late and p is not None:
        pid = _pass_id()
        if pid >= 0:
            first = getattr(_rec(p), "first", None)
            t = first[1]() if (first is not None and first[0] == pid) else None
            if t is not None and tuple(t.shape) == tuple(shape) and t.device == dev:
                r.out, r.acc = t, True
            else:
                r._first_of = p
    if r.out is None and buffer:
        r.out = torch.empty(shape, dtype=torch.float32, device=dev)
    return r


# --------------------------------------------------------------------------------------------
# device tables of the grouped launches
# --------------------------------------------------------------------------------------------
_STATIC_TABLES = _knob("SRK_NO_STATIC_TABLES", "0") != "1"      # A/B knob: descriptor tables written once per captured graph (static_tables)


class TableHolder:
    """Owns the device tables (job descriptors of the grouped launches) of hipGraphs captured under `static_tables`: keep it alive as
    long as the graphs, call `fence()` after the capture(s) and before the first replay."""

    ARENA_BYTES = 1 << 20

    def __init__(self):
        self.tables = []
        self.arena = None          # allocated by static_tables() OUTSIDE the capture: see take()
        self.used = 0

    def take(self, nbytes):
        """`nbytes` of the arena (16-byte aligned), or None when it is full.  NOT memory of the graph's own pool: an allocation made
        during the capture may reuse the address of an earlier temporary of the same graph, whose writer node would overwrite the
        table in every replay (the in-graph upload sits behind that writer; a table written once does not)."""
        n = (int(nbytes) + 15) // 16 * 16
        if self.arena is None or self.used + n > self.arena.numel():
            return None
        t = self.arena[self.used:self.used + n]
        self.used += n
        self.tables.append(t)
        return t

    def fence(self):
        if self.tables:
            L.check(L.load().srk_upload_fence(), "srk_upload_fence")


_HOLDER = None           # the TableHolder of the running static_tables block


@contextlib.contextmanager
def static_tables(holder):
    """Capture sites that own their graphs wrap the capture in this: the descriptor tables of the grouped launches (weight gradients,
    finalizes, row sums, weight normalisation) are then written ONCE, at capture time, instead of by upload launches inside the graph
    (3 per EDSR step, 30 per RCAN step at batch 16: include/srk.h, srk_upload_eager).  Valid because every address a replay sees is the
    capture's; the holder keeps the tables' memory from being reused inside the graph's pool.  Foreign captures (a user's own
    torch.cuda.graph around a step) keep the in-graph uploads."""
    ok = _STATIC_TABLES
    if ok:
        try:
            L.check(L.load().srk_upload_prepare(), "srk_upload_prepare")
        except RuntimeError:          # an older library loaded through SRK_LIB_PATH (A/B runs)
            ok = False
    if ok and holder.arena is None and not torch.cuda.is_current_stream_capturing():
        holder.arena = torch.empty(holder.ARENA_BYTES, dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
        # the arena comes from the caching allocator on the ambient stream and is written from the library's upload stream: whatever that
        # memory was last used for must have finished first (explicit, not a side effect of torch.cuda.graph's own synchronize)
        torch.cuda.current_stream().synchronize()
    global _HOLDER
    prev, _HOLDER = _HOLDER, (holder if ok else None)
    try:
        yield holder
    finally:
        _HOLDER = prev


@contextlib.contextmanager
def graph_capture(g, **kw):
    """`torch.cuda.graph(g, **kw)` for a graph whose owner is this package: the grouped launches' tables are static (static_tables),
    kept alive by the graph object itself."""
    holder = TableHolder()
    try:
        with static_tables(holder):
            with torch.cuda.graph(g, **kw):
                yield holder
    finally:
        holder.fence()
    g._srk_tables = holder


def _upload_table(host_addr, nbytes, alloc, dev, st):
    """Host bytes -> a fresh device table of `alloc` bytes on stream `st` (see static_tables)."""
    h = _HOLDER
    if h is not None and h.arena is not None and h.arena.device == torch.device(dev) and torch.cuda.is_current_stream_capturing():
        table = h.take(alloc)
        if table is not None:
            L.check(L.load().srk_upload_eager(table.data_ptr(), host_addr, nbytes), "srk_upload_eager")
            return table
    table = torch.empty(alloc, dtype=torch.uint8, device=dev)
    L.check(L.load().srk_upload_small(table.data_ptr(), host_addr, nbytes, st), "srk_upload_small")
    return table


# --------------------------------------------------------------------------------------------
# weight gradients: one launch now, or queued for the grouped launch at the end of the pass
# --------------------------------------------------------------------------------------------
def wgrad_raw(x, dy, *, N, H, W, Cin, Cout, k, w_shape, ps_r=0, scale=1.0, x_ps=0, dy_ps=0, want_bias=True, out_w=None, out_b=None):
    """dW (OIHW fp32) and db for a conv whose input was `x` and output gradient is `dy`.
    Cin/Cout are the padded storage channel counts of x / dy; w_shape the real OIHW shape.  out_w / out_b: write there."""
    _need_gpu(x)
    dev = x.device
    cout, cin, kh, kw = w_shape
    if N == 0:          # empty batch: zero gradients (the slab scratch would be uninitialised)
        return (torch.zeros(w_shape, dtype=torch.float32, device=dev),
                torch.zeros(cout, dtype=torch.float32, device=dev) if want_bias else None)
    nck = _batch_chunks(N, x, dy)
    if nck > 1:         # 2 GiB and more: sum the gradients of batch chunks (each chunk keeps the slab kernels)
        step = -(-N // nck)
        dw = db = None
        for n0 in range(0, N, step):
            n1 = min(N, n0 + step)
            w_, b_ = wgrad_raw(x[n0:n1], dy[n0:n1], N=n1 - n0, H=H, W=W, Cin=Cin, Cout=Cout, k=k, w_shape=w_shape, ps_r=ps_r,
                               scale=scale, x_ps=x_ps, dy_ps=dy_ps, want_bias=want_bias)
            dw = w_ if dw is None else dw.add_(w_)
            db = b_ if (db is None or b_ is None) else db.add_(b_)
        if out_w is not None:
            dw = out_w.copy_(dw)
        if out_b is not None and db is not None:
            db = out_b.copy_(db)
        return dw, db
    a = L.WgradArgs(x=x.data_ptr(), x_pitch=_pitch(x), x_coff=0, x_ps=int(x_ps),
                    dy=dy.data_ptr(), dy_pitch=_pitch(dy), dy_coff=0, dy_ps=int(dy_ps),
                    N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=k, KW=k, dwp=0, dbp=0, nslabs=0, dtype=_DT[x.dtype],
                    cout_real=int(cout) if (ps_r <= 1 and not x_ps and not dy_ps) else 0)
    nslabs = L.load().srk_wgrad_slabs(a)
    couts = L.load().srk_wgrad_slab_cout(a)     # channels per slab row: Cout, or 4 (compact slabs: large kernel, <= 4 real output channels)
    per = k * k * Cin * couts
    if nslabs <= 0:
        raise RuntimeError(f"srk_wgrad_slabs: no weight-gradient kernel for a {k}x{k} convolution {Cin} -> {Cout} in {x.dtype}")
    # every workgroup writes its own slab, in every dtype: nothing to zero, srk_wgrad_finalize sums the slabs in a fixed order
    scratch = torch.empty(nslabs * (per + couts), dtype=torch.float32, device=dev)
    dbp = scratch[nslabs * per:]
    a.dwp, a.dbp, a.nslabs = scratch.data_ptr(), (dbp.data_ptr() if want_bias else 0), nslabs
    L.call("srk_conv2d_wgrad", a, _stream())
    dw = out_w if out_w is not None else torch.empty(w_shape, dtype=torch.float32, device=dev)
    db = (out_b if out_b is not None else torch.empty(cout, dtype=torch.float32, device=dev)) if want_bias else None
    # the unfolded head conv presents its OIHW weight as a 1x1 conv over Cin*KH*KW channels
    f = L.WgradFinArgs(dwp=scratch.data_ptr(), dbp=dbp.data_ptr() if want_bias else 0, nslabs=nslabs, dw=dw.data_ptr(), db=_ptr(db),
                       Cout=cout, Cin=(cin * kh * kw) // (k * k), KH=k, KW=k, CinP=Cin, CoutP=couts,
                       ps_r=int(ps_r), scale=float(scale), accumulate=0)
    L.call("srk_wgrad_finalize", f, _stream())
    return dw, db


class _WgradQueue:
    """Parameter-gradient jobs of the backward pass in flight (one process per GPU: autograd's device thread appends,
    the engine's final callback -- or a gradient-bucket hook -- flushes)."""

    def __init__(self):
        self.jobs = []          # conv weight-gradient jobs (dicts), see wgrad()
        self.rjobs = []         # row-sum jobs (channel-attention parameter gradients), see defer_rowsum()
        self.armed = False      # somebody will flush (final callback queued, or inside hold_wgrads)
        self.enabled = True
        self.targets = {}       # address of a dw buffer -> number of jobs queued on it (weight sharing -> rounds)
        self.gen = 0            # queue generation (bumped by every flush or discard)
        self.stream = None      # stream of the backward pass (the flush launches there, whatever thread runs it)


_WQ = _WgradQueue()


class hold_wgrads:
    """Context manager for code that calls `wgrad` OUTSIDE an autograd backward pass (tests, micro-benchmarks): jobs are
    queued inside the block and flushed as one grouped launch when it exits."""

    def __enter__(self):
        self.prev, _WQ.armed = _WQ.armed, True
        return self

    def __exit__(self, *exc):
        _WQ.armed = self.prev
        if not self.prev and exc[0] is None:
            flush_wgrads()


class hold_wgrads_discard(hold_wgrads):
    """Like `hold_wgrads`, but the queued jobs are DROPPED on exit: a backward pass without its weight-gradient launches (bench.py times
    a trunk's data-gradient launches this way; the parameters' .grad then hold unfilled buffers -- never use them)."""

    def __exit__(self, *exc):
        discard_wgrads()
        _WQ.armed = self.prev


def set_defer_wgrad(enabled):
    """Deferral switch (default on).  Off = every weight gradient is its own launch inside backward, which is what
    code that reads gradients from inside backward needs (torch's DistributedDataParallel reducer)."""
    prev = _WQ.enabled
    _WQ.enabled = bool(enabled)
    return prev


def _arm_flush():
    """Make sure somebody flushes the queues: the autograd engine's final callback of the running backward pass."""
    if _WQ.armed:
        return True
    try:
        torch.autograd.Variable._execution_engine.queue_callback(flush_wgrads)
    except RuntimeError:            # not inside a backward pass (a Function's backward called by hand)
        return False
    _WQ.armed = True
    return True


def _launch_rowsums(rjobs, st):
    n = len(rjobs)
    host = (L.RowsumJob * n)()
    for i, j in enumerate(rjobs):
        host[i].src, host[i].dst, host[i].n, host[i].k = j["src"].data_ptr(), j["dst"], j["n"], j["k"]
    nbytes = C.sizeof(L.RowsumJob) * n
    table = _upload_table(C.addressof(host), nbytes, _roundup(nbytes, 16), rjobs[0]["src"].device, st)
    L.check(L.load().srk_rowsum_group(table.data_ptr(), n, max(j["k"] for j in rjobs), st), "srk_rowsum_group")


def defer_rowsum(per, params, shapes_offsets):
    """Sum `per` [n][K] over n into a fresh [K] buffer whose slices become the gradients of `params` -- deferred to the end of
    the backward pass, where ONE launch serves every queued job (an RCAN backward has 200 of them).

    shapes_offsets[i] = (shape, offset into the K floats) of parameter i's gradient.  Returns the list of gradient tensors
    (views of the unfilled buffer, which autograd adopts as `.grad`), or None when deferral does not apply (a gradient
    already exists and autograd would read the unfilled buffer, hooks, a second use of the parameters in this pass...)."""
    if not _WQ.enabled or per.shape[0] == 0:
        return None
    for p, (shape, _) in zip(params, shapes_offsets):
        r = route(p, shape, accumulate=True)
        if not r.late or r.acc or p is None:
            return None
        if getattr(_rec(p), "rowsum_gen", None) == _WQ.gen:
            # used twice in this pass: autograd will ADD this gradient to the (still unfilled) one queued earlier, right
            # after this backward returns -- fill the queued ones now (stream order puts the sums in front of that add)
            rj, _WQ.rjobs = _WQ.rjobs, []
            if rj:
                with torch.cuda.stream(_WQ.stream):
                    _launch_rowsums(rj, _WQ.stream.cuda_stream)
            return None
    if not _arm_flush():
        return None
    n, k = per.shape
    tot = torch.empty(k, dtype=torch.float32, device=per.device)
    stg = tot.untyped_storage()
    outs, new = [], []
    for p, (shape, off) in zip(params, shapes_offsets):
        numel = 1
        for d in shape:
            numel *= d
        v = tot[off:off + numel].view(shape)
        new.append((p, v.data_ptr(), stg, tuple(shape), off))
        _rec(p, True).rowsum_gen = _WQ.gen
        outs.append(v)
    _WQ.rjobs.append(dict(src=per, dst=tot.data_ptr(), n=int(n), k=int(k), keep=[per, stg], new=new))
    _WQ.stream = torch.cuda.current_stream()
    del tot
    return outs


def discard_wgrads():
    """Drop whatever a backward pass that did NOT end normally left queued (an exception inside backward, a failed hipGraph
    capture: the engine's final callback may never have run, so `armed` would stay set and later passes would queue jobs
    nobody flushes).  Call before starting a fresh step."""
    _WQ.jobs, _WQ.rjobs, _WQ.armed, _WQ.targets = [], [], False, {}
    _WQ.gen += 1


def flush_wgrads():
    """Launch every queued job: the row sums, then ONE grouped slab kernel per dtype and ONE grouped finalize per round."""
    jobs, _WQ.jobs, _WQ.armed, _WQ.targets = _WQ.jobs, [], False, {}
    rjobs, _WQ.rjobs = _WQ.rjobs, []
    _WQ.gen += 1
    if not jobs and not rjobs:
        return
    lib = L.load()
    stream = _WQ.stream if _WQ.stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(stream):         # the flush may run on another thread than the backward nodes: same stream
        st = stream.cuda_stream
        if rjobs:
            _launch_rowsums(rjobs, st)
        for dt in sorted({j["a"].dtype for j in jobs}):
            grp = [j for j in jobs if j["a"].dtype == dt]
            n = len(grp)
            arr = (L.WgradArgs * n)(*[j["a"] for j in grp])
            nblocks, sfl = C.c_int(0), C.c_longlong(0)
            L.check(lib.srk_wgrad_group_plan(arr, n, None, None, None, C.byref(nblocks), C.byref(sfl)), "srk_wgrad_group_plan")
            dev = grp[0]["keep"][0].device
            scratch = torch.empty(sfl.value, dtype=torch.float32, device=dev)
            jb = lib.srk_wgrad_group_job_bytes()
            off_bj = _roundup(n * jb, 16)
            off_fin = _roundup(off_bj + 4 * nblocks.value, 16)
            fin_sz = C.sizeof(L.WgradFinArgs)
            total = _roundup(off_fin + n * fin_sz, 16)
            host = (C.c_ubyte * total)()
            base = C.addressof(host)
            L.check(lib.srk_wgrad_group_plan(arr, n, scratch.data_ptr(), base, base + off_bj, C.byref(nblocks), C.byref(sfl)),
                    "srk_wgrad_group_plan")
            # finalize table ordered by round (a job that accumulates into a buffer another job of this pass writes comes later)
            order = sorted(range(n), key=lambda i: grp[i]["round"])
            rounds = {}
            for pos, i in enumerate(order):
                a, f = arr[i], grp[i]
                fa = L.WgradFinArgs(dwp=a.dwp, dbp=a.dbp or 0, nslabs=a.nslabs, dw=f["dw"], db=f["db"], Cout=f["Cout"], Cin=f["Cin"],
                                    KH=3, KW=3, CinP=a.Cin, CoutP=a.Cout, ps_r=f["ps_r"], scale=f["scale"], accumulate=f["acc"])
                C.memmove(base + off_fin + pos * fin_sz, C.addressof(fa), fin_sz)
                rounds.setdefault(f["round"], [pos, 0])[1] += 1
            table = _upload_table(base, total, total, dev, st)
            L.check(lib.srk_conv2d_wgrad_group(table.data_ptr(), table.data_ptr() + off_bj, nblocks.value, dt, st), "srk_conv2d_wgrad_group")
            # workgroups per job: one per (2 input channels x 64 output channels) tile of the largest job, 32..256
            tiles = max(((a_.Cin + 1) // 2) * ((a_.Cout + 63) // 64) for a_ in arr)
            bpj = max(32, min(256, tiles))
            for r in sorted(rounds):
                pos, cnt = rounds[r]
                L.check(lib.srk_wgrad_finalize_group(table.data_ptr() + off_fin + pos * fin_sz, cnt, bpj, st), "srk_wgrad_finalize_group")
        # a gradient autograd COPIED instead of adopting (create_graph, layout contract) holds the bytes of the then
        # unfilled buffer: refresh it from the filled one.  ('new' jobs only: .grad was None, so the copy is all it holds)
        with torch.no_grad():
            for j in jobs + rjobs:
                for p, ptr, stg, shape, off in j["new"]:
                    if p is not None and getattr(_rec(p), "proxy", False):
                        continue                    # non-leaf: the gradient went to WeightNormGroup's backward by address
                    g = p.grad if p is not None else None
                    if g is not None and g.data_ptr() != ptr and tuple(g.shape) == tuple(shape):
                        g.copy_(torch.empty(0, dtype=torch.float32, device=g.device).set_(stg, int(off), tuple(shape)))
    # `table`, `scratch`, operands and result storages are referenced by enqueued work only from here on: the caching
    # allocator re-issues a freed block on this stream behind these launches


def wgrad(x, dy, *, wparam=None, bparam=None, **kw):
    """Weight (+ bias) gradient of one conv.  3x3 16-bit convs whose parameters are leaves are QUEUED and computed by
    one grouped launch when the backward pass ends (`flush_wgrads`, the autograd engine's final callback); everything
    else runs now (`wgrad_raw`).  Returns what backward() hands to autograd for (weight, bias).

    A queued job returns EMPTY tensors that autograd adopts as `.grad` (AccumulateGrad takes over a gradient nobody else
    references); the queue keeps their storages -- not the tensors -- alive and the flush fills them by address."""
    want_bias = kw.get("want_bias", True)
    k, w_shape = kw["k"], kw["w_shape"]
    dev = x.device
    rw = route(wparam, w_shape, dev, accumulate=True, slice=True)
    rb = route(bparam, (w_shape[0],), dev, accumulate=True, slice=True, want=want_bias)
    now = dict(out_w=None if rw.acc else rw.out, out_b=None if rb.acc else rb.out)      # the immediate launch never accumulates
    if not (_WQ.enabled and k == 3 and x.dtype in (torch.bfloat16, torch.float16) and kw["N"] > 0 and kw.get("x_ps", 0) <= 1):
        return wgrad_raw(x, dy, **now, **kw)
    if not rw.late or wparam is None or (want_bias and (not rb.late or rb.acc != rw.acc)) or _batch_chunks(kw["N"], x, dy) > 1:
        return wgrad_raw(x, dy, **now, **kw)
    a = L.WgradArgs(x=x.data_ptr(), x_pitch=_pitch(x), x_coff=0, x_ps=int(kw.get("x_ps", 0)),
                    dy=dy.data_ptr(), dy_pitch=_pitch(dy), dy_coff=0, dy_ps=int(kw.get("dy_ps", 0)),
                    N=kw["N"], H=kw["H"], W=kw["W"], Cin=kw["Cin"], Cout=kw["Cout"], KH=3, KW=3, dwp=0, dbp=1 if want_bias else 0,
                    nslabs=0, dtype=_DT[x.dtype])
    if not L.load().srk_wgrad_group_ok(a):
        return wgrad_raw(x, dy, **now, **kw)
    cout, cin = w_shape[0], w_shape[1]
    ret_w = ret_b = None
    keep = [x, dy]
    new = []
    if rw.acc:
        dw_ptr, db_ptr, acc = rw.out.data_ptr(), _ptr(rb.out), 1
        keep += [rw.out, rb.out]
    else:
        rec = _rec(wparam, True)
        if rec.job is not None and rec.job[0] == _WQ.gen:     # second use of a shared weight while its first job is queued: accumulate round
            dw_ptr, db_ptr, acc = rec.job[1], rec.job[2], 1
        else:
            ret_w = rw.out if rw.out is not None else torch.empty(w_shape, dtype=torch.float32, device=dev)
            ret_b = (rb.out if rb.out is not None else torch.empty(cout, dtype=torch.float32, device=dev)) if want_bias else None
            dw_ptr, db_ptr, acc = ret_w.data_ptr(), _ptr(ret_b), 0
            sw_stg = ret_w.untyped_storage()
            keep.append(sw_stg)
            new.append((wparam, dw_ptr, sw_stg, w_shape, ret_w.storage_offset()))
            if ret_b is not None:
                sb_stg = ret_b.untyped_storage()
                keep.append(sb_stg)
                new.append((bparam, db_ptr, sb_stg, (cout,), ret_b.storage_offset()))
            rec.job = (_WQ.gen, dw_ptr, db_ptr)
    rnd = _WQ.targets.get(dw_ptr, 0)                        # jobs on one buffer finalize in successive rounds
    _WQ.targets[dw_ptr] = rnd + 1
    _WQ.jobs.append(dict(a=a, dw=dw_ptr, db=db_ptr, Cout=cout, Cin=cin, ps_r=int(kw.get("ps_r", 0)), scale=float(kw.get("scale", 1.0)),
                         acc=acc, round=rnd, keep=keep, new=new))
    _WQ.stream = torch.cuda.current_stream()
    if not _arm_flush():                # not inside a backward pass (a Function's backward called by hand)
        flush_wgrads()
    return ret_w, ret_b
