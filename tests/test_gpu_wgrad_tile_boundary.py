"""GPU tests of the tile seam of the 8-row slab-mode 3x3 weight gradient (csrc/conv_wgrad.hip: wgrad_ws_body8).

The body carries the first fragments of tile it + 1 (halo rows 0-2, gradient row 0) in registers across the tile boundary: they are read inside the
last row of tile it, behind the wait and the barrier that used to open tile it + 1, from the next buffer of the four-buffer ring; the bias words of a tile
are read one per row and added between the MFMAs.  What can go wrong there is a fragment from the wrong ring buffer, a row too early, or one read before
its DMA landed.  Shapes are chosen for the seam (one tile; 3 or 4 and 4 or 5 tiles per workgroup on a 256-CU device, the fifth wrapping the ring; ragged last
tiles; several co / ci blocks), through the grouped launch (three jobs under ops.hold_wgrads()) and the single launch (ops.wgrad_raw), in bf16 and fp16,
with the 8-row form forced in a fresh child process (SRK_DEBUG=1 SRK_WGRAD_TH=8, as tests/test_gpu_wgrad_group.py does).

 * dense random operands: dW and db within relative L2 5e-5 of the float64 gradient of the rounded operands (the bound of test_gpu_wgrad_group.py);
 * one-pixel gradients: dY is non-zero in ONE pixel, at tile row 7 or 8 (last row of a tile, first of the next) and column 15 or 16 (last column of a
   tile, first of the next), in the last image and in a middle one.  Every tap of dW is then one product of two 16-bit values plus exact zeros (exact in
   fp32: 8 + 8 or 11 + 11 mantissa bits), so dW must EQUAL the float64 product and db must equal that pixel's dY.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 8, 16, 64, 64), (43, 48, 48, 64, 64), (64, 48, 48, 64, 64), (100, 37, 23, 64, 64), (24, 24, 24, 64, 256), (24, 24, 24, 128, 64)]
DTYPES = ["bf16", "f16"]

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
    """float64 dW [co][ci][kh][kw] and db of the 'same' 3x3 conv from NHWC operands: one matrix product per tap (on the CPU)."""
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    xp = torch.zeros(n, h + 2, w + 2, cin, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x.double().cpu()
    d2 = dy.double().cpu().reshape(-1, cout)
    gw = torch.empty(cout, cin, 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            gw[:, :, kh, kw] = d2.t() @ xp[:, kh:kh + h, kw:kw + w].reshape(-1, cin)
    return gw, d2.sum(0)


def run(x, dys):
    """the grouped launch (three jobs, one per dY) and the single launch of each job"""
    n, h, w, cin = x.shape
    cout = dys[0].shape[3]
    kw = dict(N=n, H=h, W=w, Cin=cin, Cout=cout, k=3, w_shape=(cout, cin, 3, 3))
    ws = [torch.nn.Parameter(torch.zeros(cout, cin, 3, 3, device=dev)) for _ in dys]
    bs = [torch.nn.Parameter(torch.zeros(cout, device=dev)) for _ in dys]
    with ops.hold_wgrads():
        res = [ops.wgrad(x, dy, wparam=wi, bparam=bi, **kw) for dy, wi, bi in zip(dys, ws, bs)]
    single = [ops.wgrad_raw(x, dy, **kw) for dy in dys]
    torch.cuda.synchronize()
    return [(r[0].detach(), r[1].detach()) for r in res], single


out = {}
for (n, h, w, cin, cout) in SHAPES:
    key = f"{n}x{h}x{w}_{cin}_{cout}"
    g = torch.Generator().manual_seed(n * 1000 + h)
    x = (torch.rand(n, h, w, cin, generator=g) - 0.5).to(dt).to(dev)
    dy = (torch.rand(n, h, w, cout, generator=g) - 0.5).to(dt).to(dev)
    # ---- dense
    grouped, single = run(x, [dy, dy, dy])
    rw, rb = ref64(x, dy)
    rel = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())
    dense = {"rel": rel(grouped[0][0], rw), "brel": rel(grouped[0][1], rb), "rel_single": rel(single[0][0], rw), "brel_single": rel(single[0][1], rb),
             "same_jobs": bool(torch.equal(grouped[0][0], grouped[2][0]) and torch.equal(grouped[0][1], grouped[2][1]))}
    # ---- one-pixel gradients
    places = [(im, r, c) for im in sorted({n - 1, n // 2}) for r in (7, 8) for c in (15, 16) if r < h and c < w]
    xp = torch.zeros(n, h + 2, w + 2, cin, dtype=torch.float64, device=dev)
    xp[:, 1:-1, 1:-1] = x.double()
    pix = []
    for i in range(0, len(places), 3):
        trio = (places[i:i + 3] * 3)[:3]
        dys = []
        for (im, r, c) in trio:
            d1 = torch.zeros_like(dy)
            d1[im, r, c] = dy[im, r, c]
            dys.append(d1)
        grouped, single = run(x, dys)
        for (im, r, c), gr, si in list(zip(trio, grouped, single))[:len(places[i:i + 3])]:
            v = dy[im, r, c].double()                                              # [cout]
            want = (v[:, None, None, None] * xp[im, r:r + 3, c:c + 3].permute(2, 0, 1)[None])     # [cout][cin][3][3], exact in float64
            rec = {"place": [im, r, c]}
            for tag, (gw, gb) in (("grouped", gr), ("single", si)):
                rec[tag + "_dw_equal"] = bool(torch.equal(gw.double(), want))
                rec[tag + "_dw_maxdiff"] = float((gw.double() - want).abs().max())
                rec[tag + "_db_equal"] = bool(torch.equal(gb.double(), v))
                rec[tag + "_db_maxdiff"] = float((gb.double() - v).abs().max())
            rec["nonzero"] = int((want != 0).sum())
            pix.append(rec)
    out[key] = {"dense": dense, "pixel": pix}
print("RESULT " + json.dumps(out))
''' % (ROOT, SHAPES)

_CACHE = {}


def _child(dtype_name):
    """One fresh process per dtype with the 8-row form forced; its results are shared by all the cases of that dtype."""
    if dtype_name not in _CACHE:
        env = dict(os.environ, SRK_DEBUG="1", SRK_WGRAD_TH="8")
        p = subprocess.run([sys.executable, "-c", CHILD, dtype_name], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        _CACHE[dtype_name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    return _CACHE[dtype_name]


def _key(shape):
    n, h, w, cin, cout = shape
    return f"{n}x{h}x{w}_{cin}_{cout}"


@pytest.mark.parametrize("shape", SHAPES, ids=_key)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_dense_operands_against_float64(dtype_name, shape):
    r = _child(dtype_name)[_key(shape)]["dense"]
    print(dtype_name, _key(shape), r)
    assert r["rel"] < 5e-5 and r["rel_single"] < 5e-5, r
    assert r["brel"] < 5e-5 and r["brel_single"] < 5e-5, r
    assert r["same_jobs"], "the three jobs of one grouped launch had the same operands"


@pytest.mark.parametrize("shape", SHAPES, ids=_key)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_one_pixel_gradients_are_exact(dtype_name, shape):
    n, h, w, _, _ = shape
    recs = _child(dtype_name)[_key(shape)]["pixel"]
    want = [[im, r, c] for im in sorted({n - 1, n // 2}) for r in (7, 8) for c in (15, 16) if r < h and c < w]
    assert [r["place"] for r in recs] == want and recs
    for r in recs:
        print(dtype_name, _key(shape), r)
    for r in recs:
        assert r["nonzero"] > 0
        for tag in ("grouped", "single"):
            assert r[tag + "_dw_equal"], (tag, r)
            assert r[tag + "_db_equal"], (tag, r)
