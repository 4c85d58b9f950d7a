"""Packed shadow weights of the HIP hot path: the per-use packs (`pack_conv`, `pw_pack`, `proj_pack`) and a model's `PackGroup`, which
re-packs all of them in one launch per kind at the top of its forward (`forward_scope`).  Part of `ops` (re-exported there).

Ownership: a packed object must stay referenced until the launch that reads it has been enqueued (the caching allocator reuses
memory in stream order, so nothing is needed after that).  Launch wrappers keep their pack as an argument; `ops._conv_args` attaches
it to the descriptor it returns, so a table of descriptors owns its packs."""
import ctypes as C
import os
import threading
import weakref

import torch

from . import _lib as L

__all__ = ["Packed", "PwPacked", "pack_cache", "DeviceTable", "PackGroup", "forward_scope", "pack_conv", "pw_pack", "proj_pack",
           "proj_groupable", "pad16"]

_DT = {torch.bfloat16: L.SRK_BF16, torch.float16: L.SRK_F16, torch.float32: L.SRK_F32}


def _knob(name, default="0"):
    """A/B switches of tools/ (SRK_NO_PAIR, SRK_NO_HR_COLLAPSE, ...): read ONLY under SRK_DEBUG=1, so that a stray variable in a user's
    environment cannot silently route the product path through a slower diagnostic form."""
    return os.environ.get(name, default) if os.environ.get("SRK_DEBUG") == "1" else default


def pad16(c):
    return (int(c) + 15) // 16 * 16


def _roundup(a, b):
    return (a + b - 1) // b * b


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError("the sr_amd HIP ops run on an MI355X ('cuda') device only; there is no CPU fallback "
                           "(use oracle/ for a CPU reference in tests)")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _f32c(t):
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


class Packed:
    __slots__ = ("wpk", "bias", "KinP", "CoutP", "k", "ps_r", "cr")


class PwPacked:
    __slots__ = ("fwd", "bwd", "cin", "chid", "cmid", "coutp")


_PACK_CACHE_ENABLED = False


class pack_cache:
    """Context manager: reuse packed weights across calls while the parameters are FROZEN (inference loops).

    Off by default: an optimizer may update parameters without touching their autograd version counter
    (torch's fused Adam does), so a version-keyed cache cannot be trusted while training -- every forward /
    backward repacks (one small kernel per conv)."""

    def __init__(self, enabled=True):
        self.enabled, self.prev = enabled, None

    def __enter__(self):
        global _PACK_CACHE_ENABLED
        self.prev, _PACK_CACHE_ENABLED = _PACK_CACHE_ENABLED, self.enabled
        return self

    def __exit__(self, *exc):
        global _PACK_CACHE_ENABLED
        _PACK_CACHE_ENABLED = self.prev


_PACK_TILED = _knob("SRK_NO_PACK_TILED", "0") != "1"      # A/B knob: the strided-read grouped pack launch


class DeviceTable:
    """Host bytes (a launch's table of descriptors) on the device, in a buffer that keeps its ADDRESS while the content fits -- a
    captured step names it -- and grows with head room when it does not.  Rewritten only when the bytes change."""

    def __init__(self):
        self.buf, self.host = None, None

    def put(self, host, device):
        raw = bytes(host)
        if self.buf is None or self.buf.device != device or self.buf.numel() < len(raw):
            self.buf, self.host = torch.empty(max(2 * len(raw), 4096), dtype=torch.uint8, device=device), None
        if raw != self.host:
            self.buf[:len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            self.host = raw
        return self.buf


def _launch_pw(g, ents, dirty, dev):
    if dirty:
        g.table("pw").put((L.PwPackArgs * len(ents))(*[e[0] for e in ents.values()]), dev)
    L.check(L.load().srk_pw_pack_group(g.tables["pw"].buf.data_ptr(), len(ents), _stream()), "srk_pw_pack_group")


def _launch_proj(g, ents, dirty, dev):
    """All projection weights of one storage dtype -> fragment order in ONE launch."""
    by_dt = {}
    for (_, dt), e in ents.items():
        by_dt.setdefault(dt, []).append(e[0])
    for dt, jobs in by_dt.items():
        if dirty:
            g.table(("proj", dt)).put((L.ProjPackJob * len(jobs))(*jobs), dev)
        L.check(L.load().srk_proj_pack_group(g.tables[("proj", dt)].buf.data_ptr(), len(jobs), _DT[dt], _stream()), "srk_proj_pack_group")


def _launch_conv(g, ents, dirty, dev):
    n = len(ents)
    if dirty:
        arr = (L.PackArgs * n)(*[e[0] for e in ents.values()])
        tiles = (C.c_int * (n + 1))()         # blocks of the launch -> (entry, tile): prefix sums of the entries' tile counts
        L.check(L.load().srk_pack_group_tiles(C.addressof(arr), n, C.addressof(tiles)), "srk_pack_group_tiles")
        g.table("conv").put(arr, dev)
        g.table("tiles").put(tiles, dev)
        g.total_tiles = int(tiles[n])
    table = g.tables["conv"].buf.data_ptr()
    if _PACK_TILED:
        L.check(L.load().srk_pack_conv_weights_group_tiled(table, g.tables["tiles"].buf.data_ptr(), n, g.total_tiles, _stream()),
                "srk_pack_conv_weights_group_tiled")
    else:
        L.check(L.load().srk_pack_conv_weights_group(table, n, _stream()), "srk_pack_conv_weights_group")


# kind -> (descriptor fields that hold source addresses, how to read those addresses from an entry's sources, launch).
# refresh() runs the kinds in this order.
_KINDS = {
    "pw": (("w1", "b1", "w2", "b2"), lambda s: (s[0].data_ptr(), _ptr(s[1]), s[2].data_ptr(), _ptr(s[3])), _launch_pw),  # pw_chain.hip
    "proj": (("w4",), lambda s: (s[0].data_ptr(),), _launch_proj),                      # D-DBPN's projection convs (csrc/proj.hip)
    "conv": (("w", "bias"), lambda s: (s[0].data_ptr(), 0 if s[1] is None else s[1].data_ptr()), _launch_conv),   # srk_conv2d layouts
}


class PackGroup:
    """The packed shadow weights of ONE model, re-packed by a single launch per kind and step.

    `forward_scope(group)` (entered at the top of a model's forward) refreshes every (parameter, layout) the model has used so
    far -- conv forward and dgrad layouts, pointwise pairs, projections -- from device-side tables, so the ~2 pack launches per
    conv per training step collapse into one.  Entries are discovered on the first step (packed individually then).  Buffers are
    persistent, so the launches are hipGraph-capturable.  When a pack may be served from here: see `_group_for`."""

    def __init__(self):
        self.registry = {kind: {} for kind in _KINDS}   # kind -> key -> [descriptor, packed, sources, source addresses]
        # each kind's entries under the name it had before the registry (the tests read them)
        self.entries, self.pw_entries, self.proj_entries = self.registry["conv"], self.registry["pw"], self.registry["proj"]
        self.tables = {}                                  # name -> DeviceTable
        self.dirty = set()                                # kinds whose table is out of date
        self.total_tiles = 0
        self.epoch = 0          # number of refreshes so far
        self.open = False       # inside the forward window of the latest refresh

    @staticmethod
    def _held(t):
        """What an entry keeps of a source tensor: the tensor itself for a leaf (its address is re-read every refresh), a
        DETACHED alias for anything else.  A weight-normed conv's effective weight carries the grad_fn of the step that made
        it; held here, that node would keep the AccumulateGrad nodes of an eager step (created on the eager stream) alive
        into a later hipGraph capture, whose backward then ties the eager stream into the capture and hipStreamEndCapture
        crashes."""
        return t if (t is None or t.grad_fn is None) else t.detach()

    def get(self, kind, key):
        e = self.registry[kind].get(key)
        return None if e is None else e[1]

    def add(self, kind, key, desc, packed, sources):
        """Register `packed`, made by the launch `desc` describes from `sources` (whose addresses sit in `desc`)."""
        sources = tuple(self._held(t) for t in sources)
        self.registry[kind][key] = [desc, packed, sources, _KINDS[kind][1](sources)]
        self.dirty.add(kind)

    def table(self, name):
        return self.tables.setdefault(name, DeviceTable())

    def refresh(self):
        self.epoch += 1
        for kind, (fields, read, launch) in _KINDS.items():
            ents = self.registry[kind]
            if not ents:
                continue
            for e in ents.values():             # parameters moved / re-allocated since the table was built?
                addrs = read(e[2])
                if addrs != e[3]:
                    for f, a in zip(fields, addrs):
                        setattr(e[0], f, a)
                    e[3] = addrs
                    self.dirty.add(kind)
            launch(self, ents, kind in self.dirty, next(iter(ents.values()))[2][0].device)
            self.dirty.discard(kind)


_TLS = threading.local()


class forward_scope:
    """`with forward_scope(group):` around a model's forward: refreshes `group` and makes it the group that serves / registers
    packed weights until the block exits.  `group=None`: no grouping (every pack is made per use)."""

    def __init__(self, group):
        self.group = group

    def __enter__(self):
        self.prev = getattr(_TLS, "group", None)
        _TLS.group = self.group
        if self.group is not None:
            self.group.refresh()
            self.group.open = True
        return self

    def __exit__(self, *exc):
        if self.group is not None:
            self.group.open = False
        _TLS.group = self.prev


def _tok():
    """(group, epoch) token of the forward window a Function is being built in, or None."""
    g = getattr(_TLS, "group", None)
    return (weakref.ref(g), g.epoch) if (g is not None and g.open) else None


def _group_for(token):
    """The PackGroup allowed to serve a pack now, or None (pack from the current parameter values).

    A forward (token None) is served by the open forward window's group.  A backward passes the token its forward was built
    under and is served only while no later refresh has happened: the group's buffers are re-packed in place by every forward
    window, from weights an optimizer may have changed since (torch's fused Adam does not bump `_version`).  So a backward with a
    current token reads the group's buffer, with a stale token it re-packs.  With no token at all (built outside a window) the
    conv kind re-packs too, since the dgrad layout differs from the forward's, while the pw and proj kinds reuse the pack their
    forward saved: those packs carry both directions."""
    if token is not None:
        g = token[0]()
        return g if (g is not None and g.epoch == token[1]) else None
    g = getattr(_TLS, "group", None)
    return g if (g is not None and g.open) else None


def pack_conv(w, b, dtype, *, dgrad=False, ps_r=0, cache=True, as_1x1=False, token=None):
    """OIHW fp32 `w` (+ bias) -> packed shadow layout for srk_conv2d (forward or dgrad).
    as_1x1: present the OIHW weight as the 1x1 conv over Cin*KH*KW unfolded channels (head / skip convs).
    token: the (group, epoch) a Function's forward was built under (backward calls pass it: see _group_for)."""
    _need_gpu(w)
    # a weight-normed conv's effective weight (WeightNormGroup) is a non-leaf tensor in a buffer with a STABLE address: it joins
    # the grouped pack launch under the identity of its `weight_v` parameter
    kobj = None if isinstance(w, torch.nn.Parameter) else w.__dict__.get("_srk_pack_key")
    is_param = isinstance(w, torch.nn.Parameter) or kobj is not None
    key = (id(w) if kobj is None else kobj, dtype, bool(dgrad), int(ps_r), bool(as_1x1))
    group = _group_for(token) if is_param else None
    if group is not None:
        hit = group.get("conv", key)
        if hit is not None:
            return hit
    ver = (w._version, -1 if b is None else b._version, w.data_ptr())
    store = None
    if cache and _PACK_CACHE_ENABLED and is_param and kobj is None:
        store = w.__dict__.setdefault("_srk_pack", {})
        hit = store.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
    cout, cin, kh, kw = w.shape
    assert kh == kw
    if as_1x1:
        cin, kh, kw = cin * kh * kw, 1, 1
    p = Packed()
    p.k, p.ps_r = kh, int(ps_r)
    if not dgrad:
        p.KinP, p.CoutP = pad16(cin), _roundup(cout, L.conv_tile(cout))
    else:
        p.KinP, p.CoutP = pad16(cout), _roundup(cin, L.conv_tile(cin))
    wf = _f32c(w)
    # large kernel with few output channels (SRResNet's 9x9 tail, 64 -> 3): the forward kernel wants (kw, co) pairs on the MFMA rows;
    # that layout (kh * 2048 elements) rides behind the standard one
    rows = (not dgrad and not as_1x1 and kh in (5, 7, 9) and cin == 64 and cout <= 4 and cout * kw <= 32 and int(ps_r) <= 1
            and dtype in (torch.bfloat16, torch.float16) and p.CoutP == 32)
    p.cr = int(cout) if rows else 0
    p.wpk = torch.empty(kh * kw * p.KinP * p.CoutP + (kh * 2048 if rows else 0), dtype=dtype, device=w.device)
    p.bias = None
    bf = None
    if not dgrad:
        p.bias = torch.empty(p.CoutP, dtype=torch.float32, device=w.device)
        if b is not None:
            bf = _f32c(b)
    a = L.PackArgs(w=wf.data_ptr(), bias=_ptr(bf), wpk=p.wpk.data_ptr(), bias_pk=_ptr(p.bias),
                   Cout=cout, Cin=cin, KH=kh, KW=kw, KinP=p.KinP, CoutP=p.CoutP,
                   dgrad=int(dgrad), ps_r=int(ps_r), dtype=_DT[dtype], rows_layout=int(rows))
    L.call("srk_pack_conv_weights", a, _stream())
    if store is not None:
        store[key] = (ver, p)
    if group is not None and wf.data_ptr() == w.data_ptr() and (bf is None or bf.data_ptr() == b.data_ptr()):
        group.add("conv", key, a, p, (w, b if not dgrad else None))
    return p


def pw_pack(w1, b1, w2, b2, dtype, token=None):
    """fp32 [Chid][Cin][1][1] / [Cmid][Chid][1][1] (+ biases) -> the forward and backward slice streams of srk_pw_*.
    Weights with a stable identity (parameters, WeightNormGroup proxies) are served by / registered with the open PackGroup."""
    _need_gpu(w1)
    lib = L.load()
    ids = [id(w) if isinstance(w, torch.nn.Parameter) else w.__dict__.get("_srk_pack_key") for w in (w1, w2)]
    group = _group_for(token) if all(i is not None for i in ids) else None
    key = (ids[0], ids[1], dtype)
    if group is not None:
        hit = group.get("pw", key)
        if hit is not None:
            return hit
    p = PwPacked()
    p.cin, p.chid, p.cmid = int(w1.shape[1]), int(w1.shape[0]), int(w2.shape[0])
    p.coutp = _roundup(p.cmid, 64)
    p.fwd = torch.empty(lib.srk_pw_pack_bytes(p.cin, p.chid, p.coutp, 0), dtype=torch.uint8, device=w1.device)
    p.bwd = torch.empty(lib.srk_pw_pack_bytes(p.cin, p.chid, p.coutp, 1), dtype=torch.uint8, device=w1.device)
    w1f, w2f = _f32c(w1), _f32c(w2)
    b1f = None if b1 is None else _f32c(b1)
    b2f = None if b2 is None else _f32c(b2)
    a = L.PwPackArgs(w1=w1f.data_ptr(), b1=_ptr(b1f), w2=w2f.data_ptr(), b2=_ptr(b2f), Cin=p.cin, Chid=p.chid,
                     Cmid=p.cmid, CoutP=p.coutp, fwd=p.fwd.data_ptr(), bwd=p.bwd.data_ptr(), dtype=_DT[dtype])
    L.call("srk_pw_pack", a, _stream())
    if (group is not None and w1f.data_ptr() == w1.data_ptr() and w2f.data_ptr() == w2.data_ptr()
            and (b1 is None or b1f.data_ptr() == b1.data_ptr()) and (b2 is None or b2f.data_ptr() == b2.data_ptr())):
        group.add("pw", key, a, p, (w1, b1, w2, b2))
    return p


def proj_groupable(w):
    """Whether a projection weight may live in a PackGroup: a plain fp32 parameter (its address is what the group re-reads)."""
    return isinstance(w, torch.nn.Parameter) and w.dtype == torch.float32 and w.is_contiguous()


def proj_pack(w, dtype, device, token=None):
    """D-DBPN's projection weight (fp32 [32][32][8][8], csrc/proj.hip) -> the fragment orders of both directions, one half each
    (uint8 buffer).  A groupable weight is served by / registered with the open PackGroup."""
    group = _group_for(token) if proj_groupable(w) else None
    key = (id(w), dtype)
    hit = group.get("proj", key) if group is not None else None
    if hit is not None and hit.device == device:
        return hit
    lib = L.load()
    wpk = torch.empty(2 * (lib.srk_proj_pack_bytes() // 2), dtype=torch.uint8, device=device)
    w4 = _f32c(w)
    L.check(lib.srk_proj_pack(w4.data_ptr(), wpk.data_ptr(), _DT[dtype], _stream()), "srk_proj_pack")
    if group is not None:
        group.add("proj", key, L.ProjPackJob(w4=w4.data_ptr(), wpk=wpk.data_ptr()), wpk, (w,))
    return wpk
