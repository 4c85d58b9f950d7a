"""GPU tests of the helper waves of the 8-row slab-mode 3x3 weight gradient (csrc/conv_wgrad.hip: wgrad_ws_body8).

The 8-row form runs two waves per SIMD: waves 0-3 read fragments and issue MFMAs, waves 4-7 issue the LDS-DMA of the tile three ahead and sum the bias
from the gradient tile in LDS; the two roles meet at one barrier per tile.  What is new to go wrong: a helper and a compute wave disagreeing about a
tile (ring slot, past-the-end tiles), a read before the barrier that publishes it, the bias taken from the wrong buffer or by the wrong lane, LDS left
over from an earlier launch.  Shapes (on a 256-CU device): N = 16, 32, 64 at 48 x 48, 64 -> 64 give workgroups 1 or 2, 2 or 3 and 4 or 5 tiles (ring
start, the edge of the three tiles in flight, ring wrap); 100 x 37 x 23 has ragged rows and columns; 128 -> 64 has workgroups with ci block 1, which
carry no bias; 64 -> 256 has four co blocks.  Every shape runs through the grouped launch -- three jobs, the middle one WITHOUT a bias, so one launch
mixes both kinds of workgroup -- and through the single launch, in bf16 and fp16, with the 8-row form forced in a fresh child process per dtype
(SRK_DEBUG=1 SRK_WGRAD_TH=8, as tests/test_gpu_wgrad_tile_boundary.py does).

 * integer operands: x and dY take integer values in [-4, 4], so every product and every partial sum is exact in fp32 whatever the order
   (|sum| <= 16 * pixels < 2^24 for these shapes): dW and db must EQUAL the float64 result -- any missing, doubled or stale pixel shows;
 * dense random operands: dW and db within relative L2 5e-5 of the float64 gradient of the rounded operands (the bound of test_gpu_wgrad_group.py);
 * back to back: the integer launches and the dense launches of all shapes run in one process, one after the other with different data, each checked;
   one shape runs its integer case a second time with other data right behind the first.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(16, 48, 48, 64, 64), (32, 48, 48, 64, 64), (64, 48, 48, 64, 64), (100, 37, 23, 64, 64), (24, 24, 24, 128, 64), (24, 24, 24, 64, 256)]
DTYPES = ["bf16", "f16"]
KINDS = ["int", "int_again", "dense"]

CHILD = r'''
import json, sys, torch
sys.path.insert(0, %r)
import sr_amd as A
ops = A.ops
name = sys.argv[1]
dt = {"bf16": torch.bfloat16, "f16": torch.float16}[name]
SHAPES = %r
dev = torch.device("cuda")


def ref64(x, dy):
    """float64 dW [co][ci][kh][kw] and db of the 'same' 3x3 conv from NHWC operands: one float64 matrix product per tap"""
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    xp = torch.zeros(n, h + 2, w + 2, cin, dtype=torch.float64, device=x.device)
    xp[:, 1:-1, 1:-1] = x.double()
    d2 = dy.double().reshape(-1, cout)
    gw = torch.empty(cout, cin, 3, 3, dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            gw[:, :, kh, kw] = d2.t() @ xp[:, kh:kh + h, kw:kw + w].reshape(-1, cin)
    return gw, d2.sum(0)


def run(x, dy, dy2):
    """one grouped launch of three jobs -- (dy, bias), (dy, NO bias), (dy2, bias) -- and the single launch of (dy, bias)"""
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    kw = dict(N=n, H=h, W=w, Cin=cin, Cout=cout, k=3, w_shape=(cout, cin, 3, 3))
    ws = [torch.nn.Parameter(torch.zeros(cout, cin, 3, 3, device=dev)) for _ in range(3)]
    bs = [torch.nn.Parameter(torch.zeros(cout, device=dev)) for _ in range(3)]
    with ops.hold_wgrads():
        r0 = ops.wgrad(x, dy, wparam=ws[0], bparam=bs[0], **kw)
        r1 = ops.wgrad(x, dy, wparam=ws[1], bparam=None, want_bias=False, **kw)
        r2 = ops.wgrad(x, dy2, wparam=ws[2], bparam=bs[2], **kw)
    single = ops.wgrad_raw(x, dy, **kw)
    torch.cuda.synchronize()
    assert A._lib.load().srk_last_kernel().decode() == "wgrad_ws", A._lib.load().srk_last_kernel()
    return r0, r1, r2, single


def check(x, dy, dy2, exact):
    r0, r1, r2, single = run(x, dy, dy2)
    rw, rb = ref64(x, dy)
    rw2, rb2 = ref64(x, dy2)
    rec = {"nobias_db_is_none": r1[1] is None}
    for tag, gw, gb, ww, wb in (("grouped", r0[0], r0[1], rw, rb), ("grouped_nobias", r1[0], None, rw, None), ("grouped_third", r2[0], r2[1], rw2, rb2),
                                ("single", single[0], single[1], rw, rb)):
        gw = gw.detach().double()
        rec[tag + "_dw_equal"] = bool(torch.equal(gw, ww))
        rec[tag + "_dw_rel"] = float((gw - ww).norm() / ww.norm())
        rec[tag + "_dw_maxdiff"] = float((gw - ww).abs().max())
        if wb is not None:
            gb = gb.detach().double()
            rec[tag + "_db_equal"] = bool(torch.equal(gb, wb))
            rec[tag + "_db_rel"] = float((gb - wb).norm() / wb.norm())
            rec[tag + "_db_maxdiff"] = float((gb - wb).abs().max())
    rec["bound_2p24"] = bool(16 * x.shape[0] * x.shape[1] * x.shape[2] < 2 ** 24)
    return rec


out = {}
for si, (n, h, w, cin, cout) in enumerate(SHAPES):
    key = f"{n}x{h}x{w}_{cin}_{cout}"
    g = torch.Generator().manual_seed(n * 1000 + h)
    ints = lambda c: torch.randint(-4, 5, (n, h, w, c), generator=g).to(dt).to(dev)
    out[key] = {"int": check(ints(cin), ints(cout), ints(cout), True)}
    # right behind it, the same launches with other data (one shape: the ring-wrap one)
    out[key]["int_again"] = check(ints(cin), ints(cout), ints(cout), True) if si == 2 else None
    dense = lambda c: (torch.rand(n, h, w, c, generator=g) - 0.5).to(dt).to(dev)
    out[key]["dense"] = check(dense(cin), dense(cout), dense(cout), False)
print("RESULT " + json.dumps(out))
''' % (ROOT, SHAPES)

_CACHE = {}


def _child(dtype_name):
    """One fresh process per dtype with the 8-row form forced; its results are shared by all the cases of that dtype."""
    if dtype_name not in _CACHE:
        env = dict(os.environ, SRK_DEBUG="1", SRK_WGRAD_TH="8")
        p = subprocess.run([sys.executable, "-c", CHILD, dtype_name], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        _CACHE[dtype_name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    return _CACHE[dtype_name]


def _key(shape):
    n, h, w, cin, cout = shape
    return f"{n}x{h}x{w}_{cin}_{cout}"


LAUNCHES = ["grouped", "grouped_nobias", "grouped_third", "single"]


@pytest.mark.parametrize("shape", SHAPES, ids=_key)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_integer_operands_equal_float64(dtype_name, shape):
    for kind in ("int", "int_again"):
        r = _child(dtype_name)[_key(shape)][kind]
        if kind == "int_again" and shape != SHAPES[2]:
            assert r is None
            continue
        print(dtype_name, _key(shape), kind, r)
        assert r["bound_2p24"], "the shape is too large for exact fp32 sums"
        assert r["nobias_db_is_none"]
        for tag in LAUNCHES:
            assert r[tag + "_dw_equal"], (kind, tag, r)
            if tag != "grouped_nobias":
                assert r[tag + "_db_equal"], (kind, tag, r)


@pytest.mark.parametrize("shape", SHAPES, ids=_key)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_dense_operands_against_float64(dtype_name, shape):
    r = _child(dtype_name)[_key(shape)]["dense"]
    print(dtype_name, _key(shape), r)
    assert r["nobias_db_is_none"]
    for tag in LAUNCHES:
        assert r[tag + "_dw_rel"] < 5e-5, (tag, r)
        if tag != "grouped_nobias":
            assert r[tag + "_db_rel"] < 5e-5, (tag, r)
